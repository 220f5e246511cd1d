"""vvcgpu_intra_tu_code_dq_batch without a GPU: the restatement of the pass (tests/intra_tu_dq_cases.py) reproduces the compiled reference's values
(tests/golden/intra_tu_dq.npz), the file covers what it is meant to cover, the case builders of the GPU tests keep their own conditions, and the argument
checks that come before any device work answer as the header says."""
import ctypes as C
import re

import numpy as np
import pytest

import intra_mode_cand_cases as imc
import intra_tu_dq_cases as tdq
import rd_pass_kit as kit
from vvcsoftware_vtm_amd import abi, capi


@pytest.mark.parametrize("bd", [8, 10])
def test_restatement_reproduces_the_golden_file(bd):
    g = np.load(tdq.GOLDEN)
    case, flags = tdq.golden_case(g, bd)
    assert flags == tdq.WRITE_PRED
    want = tdq.restate(case, flags)
    for name in ("pred", "rec", "level", "abs_sum", "num_sig", "dist"):
        assert np.array_equal(want[name], g["bd%d_want_%s" % (bd, name)]), name
    # what the file covers: all 25 shapes with DCT-II, the four EMT pairs on the squares 4 .. 32 and EMT pairs on rectangles, luma and chroma tables, QPs
    # 22 .. 37 and the largest, at least four rate tables, two given predictions, both filter decisions, items with levels and the early return
    it = case.tc.items
    dct = (it["tr_hor"] == 0) & (it["tr_ver"] == 0)
    assert {(int(w), int(h)) for w, h in zip(it["w"][dct], it["h"][dct])} == set(imc.all_shapes())
    for s in (4, 8, 16, 32):
        sq = it[(it["w"] == s) & (it["h"] == s)]
        assert {(a, b) for a in (1, 2) for b in (1, 2)} <= {(int(a), int(b)) for a, b in zip(sq["tr_hor"], sq["tr_ver"])}
    assert ((it["w"] != it["h"]) & ~dct).sum() >= 4
    assert set(case.dq["luma"]) == {0, 1} and (it["level_off"] % 16 == 0).all()
    off = 6 * (bd - 8)
    assert {22 + off, 27 + off, 32 + off, 37 + off, 63 + off} <= {int(q) for q in it["qp"]}
    assert len({case.rates[int(i)].tobytes() for i in case.dq["rates_idx"]}) >= 4
    assert (it["mode"] == tdq.PRED_GIVEN).sum() == 2 and {int(v) for v in it["filt"][it["mode"] >= 0]} == {0, 1}
    served = want["abs_sum"] != tdq.U32_MAX
    assert served.all() and (want["abs_sum"] > 0).sum() * 3 >= served.sum() and (want["abs_sum"] == 0).any()
    assert np.array_equal(want["num_sig"] == 0, want["abs_sum"] == 0)


def test_golden_file_holds_data_only_and_stays_small():
    kit.check_golden_file(tdq.GOLDEN)


@pytest.mark.parametrize("bd", [8, 10])
def test_conditions_of_the_random_list(bd):
    """every skip kind occurs between served neighbours, more than 250 items are served, at least a third of the served items have abs_sum > 0"""
    case, lists, want = tdq.random_case(bd)
    tdq.check_random(case, tdq.random_kinds(len(case.tc.items)), want)
    skipped = want["abs_sum"] == tdq.U32_MAX
    pred0, rec0, level0 = case.tc.initial()
    assert np.array_equal(want["pred"], pred0) and (want["mode_out"][skipped] == -1).all() and (want["dist"][skipped] == tdq.U64_MAX).all()
    for i in np.flatnonzero(skipped):                                        # nothing of a skipped item is touched
        lo = int(case.tc.items[i]["level_off"])
        if lo + 64 * 64 <= case.tc.level_size:                               # (the item whose levels leave the extent points into its neighbours' regions)
            assert (want["level"][lo:lo + 16] == level0[lo:lo + 16]).all()


def test_conditions_of_the_other_builders():
    for bd in (8, 10):
        case, want = tdq.zero_case(bd)
        tdq.check_zero(case, want)
        case, want = tdq.shapes_case(bd)
        assert (want["abs_sum"] != tdq.U32_MAX).all() and (want["abs_sum"] > 0).sum() * 2 >= len(want["abs_sum"])
        tdq.clip_case(bd)
    for served in (1, 15, 16, 17, 63, 64, 65):
        case, want = tdq.count_case(served)
        assert (want["abs_sum"] != tdq.U32_MAX).sum() == served
    case, want = tdq.all_skipped_case()
    assert all(np.array_equal(want[k], b) for k, b in zip(("pred", "rec", "level"), case.tc.initial()))
    (c1, _), (c2, _) = tdq.workspace_cases()
    assert {(64, 64), (64, 16), (16, 64)} <= {(int(w), int(h)) for w, h in zip(c1.tc.items["w"], c1.tc.items["h"])}
    assert set(c1.tc.items["level_off"]) & set(c2.tc.items["level_off"])


def test_conditions_of_the_long_list():
    """on 256 compute units: 7000 items, every wavefront of every workgroup with at least two of them and differing numbers of served ones; the copied
    expectation agrees with the restatement of a sample (asserted by the builder); a prefix's expectation leaves the later items' regions alone"""
    case, lists, want = tdq.waves_case(256)
    assert len(case.tc.items) == 7000 and tdq.wave_lengths(256) == [255, 256, 257, 3071, 3072, 3073]
    tdq.check_waves(case, want, 256)
    assert set(tdq.wave_of(257, 256)) == set(range(0, 12 * 256, 12)) | {1} and tdq.wave_of(3073, 256)[-1] == 0
    idx = np.arange(40)
    head, sub = tdq.prefix_of(case, want, 40), tdq.restate(case.sub(idx), mode_list=lists)
    assert all(np.array_equal(head[k], sub[k]) for k in ("pred", "rec", "level", "abs_sum", "num_sig", "dist", "mode_out"))
    small, _, _ = tdq.waves_case(8)                                          # (a device with fewer compute units gets a shorter list by the same rule)
    assert len(small.tc.items) == 27 * 8 + 88


def test_contract_of_the_restatement():
    """what the restatement skips, item by item"""
    rng = np.random.default_rng(6)
    base = tdq.itc.fresh_base(rng, 10, [(8, 8), (64, 16)])
    specs = [dict(pu=0), dict(pu=0, level_misalign=4), dict(pu=0, level_misalign=8), dict(pu=0, level_misalign=12), dict(pu=0, level_beyond=True), dict(pu=0, rates_idx=8),
             dict(pu=0, rates_idx=-1), dict(pu=0, lam=0.0), dict(pu=0, lam=-3.0), dict(pu=1, tr_ver=2), dict(pu=1, tr_hor=2), dict(pu=0, w=4), dict(pu=0, mode=67),
             dict(pu=0, mode=tdq.FROM_LIST, row=0, slot=0), dict(pu=0, mode=tdq.PRED_GIVEN), dict(pu=0, rates_idx=7)]
    case = tdq.make(base, specs, rng)
    served = tdq.restate(case)["abs_sum"] != tdq.U32_MAX
    assert served.tolist() == [True] + [False] * 8 + [True] + [False] * 4 + [True, True]
    lists = np.full((1, 16), -1, np.int32)
    lists[0, 0], lists[0, 5] = 1, 50
    got = tdq.restate(case, mode_list=lists, have_pred=False)
    assert (got["abs_sum"] != tdq.U32_MAX).tolist() == [True] + [False] * 8 + [True] + [False] * 3 + [True, False, True] and got["mode_out"][13] == 50
    case.tc.items[0]["level_off"] = -16
    assert tdq.restate(case)["abs_sum"][0] == tdq.U32_MAX


WS = 1 << 20


def call(**kw):
    """the entry with arguments that pass every check (dummy non-null pointers: no check dereferences one), changed by kw"""
    P = C.c_void_p(64)
    a = dict(refs=P, preds=P, org=P, pred=None, rec=P, level=P, extent=1024, tus=P, dq=P, n=3, mode_list=None, rates=P, n_rates=4, quantiser=1, flags=0, bd=10,
             cmin=0, cmax=1023, abs_sum=P, num_sig=P, dist=P, mode_out=P, ws=P, ws_bytes=WS)
    a.update(kw)
    return capi.lib().vvcgpu_intra_tu_code_dq_batch(a["refs"], a["preds"], a["org"], a["pred"], a["rec"], a["level"], a["extent"], a["tus"], a["dq"], a["n"],
                                                    a["mode_list"], a["rates"], a["n_rates"], a["quantiser"], a["flags"], a["bd"], a["cmin"], a["cmax"],
                                                    a["abs_sum"], a["num_sig"], a["dist"], a["mode_out"], a["ws"], a["ws_bytes"], None)


E_ARG_CASES = [dict(n=-1), dict(refs=None), dict(preds=None), dict(org=None), dict(rec=None), dict(level=None), dict(tus=None), dict(dq=None), dict(rates=None),
               dict(abs_sum=None), dict(num_sig=None), dict(dist=None), dict(mode_out=None), dict(ws=None), dict(flags=4), dict(flags=-1), dict(flags=1),
               dict(flags=3), dict(cmin=5, cmax=4), dict(cmax=40000), dict(cmin=-40000), dict(preds=C.c_void_p(72)), dict(tus=C.c_void_p(72)), dict(dq=C.c_void_p(68)),
               dict(n_rates=0), dict(n_rates=-2), dict(extent=8), dict(ws=C.c_void_p(72)), dict(ws_bytes=1024 * 30 + 3 * 44)]


def test_argument_errors_come_before_any_device_work():
    lib = capi.lib()
    kit.check_argument_errors(call, E_ARG_CASES, b"intra_tu_code_dq_batch",
                              empty=({}, dict(refs=None, preds=None, org=None, rec=None, level=None, tus=None, dq=None, rates=None, ws=None, ws_bytes=0, quantiser=7)))
    # the workspace: coefficients, decisions, histories and parked predictions by the level extent (4 + 16 + 8 + 2 bytes each, the extent rounded up to 16), a record
    # and a work-list entry per item
    f = lib.vvcgpu_intra_tu_code_dq_workspace_bytes
    assert f(160, 0) - f(16, 0) == 144 * 30 and f(17, 3) == f(32, 3) and f(32, 4) - f(32, 3) == 40 + 4
    # absolutely: 16 * 30 and the slack of 4096 * 4 + 256; further pairs as the library gave them before the layout was stated once (dqpass_dev.h)
    assert f(16, 0) == 16 * 30 + 16640 == 17120
    assert [f(e, n) for e, n in ((17, 3), (33, -2), (1000, 5), (4096, 3), (65551, 7), (100000, 1000))] == [17732, 18080, 47100, 139652, 1983508, 3060640]
    assert call(ws_bytes=f(1024, 3) - 1) == -1
    for q in (0, 2, -1):                                                     # a quantiser other than the served one
        assert call(quantiser=q) == -3, q
        assert b"quantiser" in lib.vvcgpu_last_error(), q


def test_abi_of_the_entry():
    """the constant mirrors the header, the prototypes are read from it, and the header has no struct of the entry's own"""
    hdr = " ".join(open(capi.HEADER).read().split())
    assert int(re.search(r"#define VVCGPU_INTRA_TU_Q_DEPQUANT (\d+)", hdr).group(1)) == abi.INTRA_TU_Q_DEPQUANT == 1
    protos = capi.prototypes()
    assert len(protos["vvcgpu_intra_tu_code_dq_batch"][1]) == 25 and protos["vvcgpu_intra_tu_code_dq_workspace_bytes"] == (C.c_size_t, (C.c_size_t, C.c_int))
    assert protos["vvcgpu_intra_tu_code_dq_batch"][1][6] is C.c_size_t and protos["vvcgpu_intra_tu_code_dq_batch"][1][23] is C.c_size_t
