"""vvcgpu_intra_chroma_code_dq_batch without a GPU: the restatement of the pass (tests/intra_chroma_dq_cases.py) keeps the entry's contract, the seeded cases
meet the conditions that make a wrong choice of the Cr record show, and the argument checks that come before any device work, the workspace-size
arithmetic and the prototype answer as the header says."""
import ctypes as C
import re

import numpy as np
import pytest

import intra_chroma_dq_cases as cdq
import rd_pass_kit as kit
from test_intra_chroma_code_cpu import E_ARG_CASES as SIBLING_E_ARG
from vvcsoftware_vtm_amd import abi, capi


def test_contract_of_the_restatement():
    """each skip kind alone skips the whole PU and leaves its neighbours as they were: a 2-sample run, level_off 4 / 8 / 12 / negative, beyond the extent,
    each of the three records bad; a PU that ends at the extent is served"""
    rng = np.random.default_rng(5)
    specs = [dict(w=4, h=4), dict(w=4, h=8), dict(w=8, h=8), dict(w=8, h=8), dict(w=2, h=8)]
    full_case = cdq.make(rng, 10, specs)
    full = cdq.restate(full_case)
    served = (full["abs_sum"] != cdq.U32_MAX).any(axis=(1, 2))
    assert list(served) == [False, True, True, True, True] and (full_case.cc.runs[0, :2] == (2, 8)).all()     # (make groups by shape: the 2 x 8 run comes first)

    def alone(change):
        case = cdq.Case(full_case.cc.sub(np.arange(5)), full_case.dq.copy(), full_case.rates)
        change(case)
        got = cdq.restate(case)
        assert (got["abs_sum"][2] == cdq.U32_MAX).all() and (got["dist"][2] == cdq.U64_MAX).all()
        for q in (1, 3, 4):
            assert np.array_equal(got["abs_sum"][q], full["abs_sum"][q]) and np.array_equal(got["dist"][q], full["dist"][q])
        u = full_case.cc.pus[2]
        lo, co, size = int(u["level_off"]), int(u["cand_off"]), 12 * int(u["w"]) * int(u["h"])
        assert (got["level"][lo:lo + size] == kit.LEVEL_CANARY).all() and (got["rec"][co:co + size] == kit.REC_CANARY).all()

    for off in (4, 8, 12):
        alone(lambda c, off=off: c.cc.pus["level_off"].__setitem__(2, c.cc.pus["level_off"][2] + off))
    alone(lambda c: c.cc.pus["level_off"].__setitem__(2, -16))
    alone(lambda c: c.cc.pus["level_off"].__setitem__(2, c.cc.level_size - 12 * 4 * 8 + 16))
    for j in range(3):
        alone(lambda c, j=j: c.dq["rates_idx"].__setitem__(3 * 2 + j, len(c.rates)))
        alone(lambda c, j=j: c.dq["rates_idx"].__setitem__(3 * 2 + j, -1))
        alone(lambda c, j=j: c.dq["lambda"].__setitem__(3 * 2 + j, 0.0))
        alone(lambda c, j=j: c.dq["luma"].__setitem__(3 * 2 + j, 1))
    fits = cdq.Case(full_case.cc.sub(np.arange(5)), full_case.dq.copy(), full_case.rates)
    fits.cc.pus["level_off"][4] = fits.cc.level_size - 12 * 8 * 8
    assert cdq.pu_ok(fits, 4)


@pytest.mark.parametrize("bd", [8, 10])
def test_random_case_meets_its_conditions(bd):
    case, kinds, want = kit.cached(cdq.random_case, bd)                      # (the builder asserts them)
    assert set(k for k in kinds if k) == set(cdq.SKIP_KINDS)


def call(**kw):
    """the entry with arguments that pass every check (dummy non-null pointers: no check dereferences one), changed by kw"""
    runs = np.array(kw.pop("runs", [[8, 8, 3]]), np.int32)
    f = capi.lib().vvcgpu_intra_chroma_code_dq_workspace_bytes
    a = dict(rec=None, flags_base=None, fill=None, refs=C.c_void_p(64), luma=None, org=C.c_void_p(64), pus=C.c_void_p(64), dq=C.c_void_p(64), n=3, n_runs=len(runs),
             rates=C.c_void_p(64), n_rates=2, quantiser=1, pred=None, cand_rec=C.c_void_p(64), level=C.c_void_p(64), extent=4096, flags=0, bd=10, cmin=0, cmax=1023,
             abs_sum=C.c_void_p(64), dist=C.c_void_p(64), ws=C.c_void_p(64), ws_bytes=f(4096, 3), runs_ptr=runs.ctypes.data_as(C.c_void_p))
    a.update(kw)
    return capi.lib().vvcgpu_intra_chroma_code_dq_batch(a["rec"], a["flags_base"], a["fill"], a["refs"], a["luma"], a["org"], a["pus"], a["dq"], a["n"], a["runs_ptr"],
                                                        a["n_runs"], a["rates"], a["n_rates"], a["quantiser"], a["pred"], a["cand_rec"], a["level"], a["extent"], a["flags"],
                                                        a["bd"], a["cmin"], a["cmax"], a["abs_sum"], a["dist"], a["ws"], a["ws_bytes"], None)


E_ARG_CASES = SIBLING_E_ARG + [dict(dq=None), dict(rates=None), dict(ws=None), dict(n_rates=0), dict(n_rates=-1), dict(extent=15), dict(extent=0), dict(dq=C.c_void_p(68)),
                               dict(ws=C.c_void_p(72)), dict(ws_bytes=0), dict(n=(2 ** 31 - 1) // 12 + 1, runs=[[8, 8, (2 ** 31 - 1) // 12 + 1]]),
                               dict(extent=1 << 40, ws_bytes=1 << 62)]


def test_argument_errors_come_before_any_device_work():
    kit.check_argument_errors(call, E_ARG_CASES, b"intra_chroma_code_dq_batch", empty=({}, dict(org=None, pus=None, runs_ptr=None, dq=None, rates=None, ws=None)))
    lib = capi.lib()
    for q in (0, 2, -1):
        assert call(quantiser=q) == -3 and b"intra_chroma_code_dq_batch" in lib.vvcgpu_last_error()
    f = lib.vvcgpu_intra_chroma_code_dq_workspace_bytes
    assert f(160, 0) - f(16, 0) == 144 * 30 and f(17, 3) == f(32, 3) and f(32, 4) - f(32, 3) == 12 * (40 + 4) and f(16, -1) == f(16, 0)
    # absolutely: 16 * 30 and the slack of 4096 * 4 + 256; further pairs as the library gave them before the layout was stated once (dqpass_dev.h)
    assert f(16, 0) == 16 * 30 + 16640 == 17120
    assert [f(e, n) for e, n in ((17, 3), (33, -2), (1000, 5), (4096, 3), (65551, 7), (100000, 1000))] == [19184, 18080, 49520, 141104, 1986896, 3544640]
    assert call(ws_bytes=f(4096, 3) - 1) == -1 and call(extent=4097, ws_bytes=f(4096, 3)) == -1


def test_the_python_side_mirrors_the_header():
    """the constant mirrors the header and the prototypes are read from it (tests/test_abi.py checks that the header has no struct beyond its mirrors)"""
    hdr = " ".join(open(capi.HEADER).read().split())
    assert int(re.search(r"#define VVCGPU_INTRA_CHROMA_Q_DEPQUANT (\d+)", hdr).group(1)) == abi.INTRA_CHROMA_Q_DEPQUANT == 1
    protos = capi.prototypes()
    args = protos["vvcgpu_intra_chroma_code_dq_batch"][1]
    assert len(args) == 27 and args[17] is C.c_size_t and args[25] is C.c_size_t
    assert protos["vvcgpu_intra_chroma_code_dq_workspace_bytes"] == (C.c_size_t, (C.c_size_t, C.c_int))


@pytest.mark.parametrize("bd", [8, 10])
def test_restatement_reproduces_the_golden_file(bd):
    g = np.load(cdq.GOLDEN)
    case, flags = cdq.golden_case(g, bd)
    assert flags == cdq.WRITE_PRED
    want = cdq.restate(case, flags)
    for name in ("refs", "pred", "rec", "level", "abs_sum", "dist"):
        assert np.array_equal(want[name], g["bd%d_want_%s" % (bd, name)]), name
    cdq.golden_conditions(case, want)                                        # both Cb outcomes, the Cr items that tell the records apart, tables, QPs, slots


def test_golden_file_holds_data_only_and_stays_small():
    kit.check_golden_file(cdq.GOLDEN)


def test_the_other_seeded_cases_meet_their_conditions():
    """the builders assert them: the all-zero items, the two lists of one workspace, the copies of the wavefront lists"""
    cdq.zero_case(8), cdq.zero_case(10), cdq.workspace_cases(), cdq.waves_case(100), cdq.mixed_case(10)
