"""vvcgpu_intra_tu_code_batch without a device: the restatement of the pass (tests/intra_tu_code_cases.py) against the reference's values
(tests/golden/intra_tu_code.npz), the conditions the case builders promise -- the caps on all-zero items and skipped slots, an empty and a full list, the
bound items -- and the argument checks the entry makes before any device work."""
import ctypes as C

import numpy as np
import pytest

import intra_mode_cand_cases as imc
import intra_tu_code_cases as itc
from vvcsoftware_vtm_amd import capi


@pytest.mark.parametrize("bd", [8, 10])
def test_restatement_equals_golden(bd):
    g = np.load(itc.GOLDEN)
    tc, flags = itc.golden_case(g, bd)
    got = itc.restate(tc, flags)
    k = "bd%d_want_" % bd
    for name in ("pred", "rec", "level", "abs_sum", "num_sig", "dist"):
        assert np.array_equal(got[name], g[k + name]), name
    it = tc.items
    assert {(int(a), int(b)) for a, b in zip(it["w"], it["h"])} == set(imc.all_shapes())
    assert {0, 1, 2, 18, 34, 50, 66} <= {int(m) for m in it["mode"]} and any(m > 2 and m & 1 for m in it["mode"]) and (it["mode"] == itc.PRED_GIVEN).any()
    assert any(imc.wide_angle(int(a), int(b), int(m)) != m for a, b, m in zip(it["w"], it["h"], it["mode"]) if m >= 0)
    assert {0, 1} == {int(f) for f in it["filt"][it["mode"] >= 0]}
    itc.check_conditions(tc, got)


@pytest.mark.parametrize("bd", [8, 10])
def test_conditions_of_the_random_cases(bd):
    tc, want = itc.shapes_case(bd)                                            # (asserts the cap on all-zero items itself)
    it = tc.items
    assert {(int(a), int(b)) for a, b in zip(it["w"], it["h"])} == set(imc.all_shapes())
    assert {0, itc.max_qp(bd)} <= {int(q) for q in it["qp"]} and {0, 1} == {int(v) for v in it["sbh"]} == {int(v) for v in it["intra"]}
    small = [(int(a), int(b)) for a, b, c, d in zip(it["tr_hor"], it["tr_ver"], it["w"], it["h"]) if c <= 32 and d <= 32]
    assert set(small) == {(0, 0), (1, 1), (1, 2), (2, 1), (2, 2)}
    assert (want["abs_sum"] != itc.U32_MAX).all() and np.array_equal(want["mode_out"], it["mode"])
    base, cand, tc, want = itc.handover_case(bd)                              # (asserts the cap on skipped slots, an empty and a full list)
    sizes = cand["lists"][:, 0]
    skipped = want["abs_sum"] == itc.U32_MAX
    assert np.array_equal(skipped, tc.items["slot"] >= sizes[tc.items["row"]])
    assert (want["num_sig"][skipped] == itc.U32_MAX).all() and (want["dist"][skipped] == itc.U64_MAX).all() and (want["mode_out"][skipped] == -1).all()


@pytest.mark.parametrize("bd", [8, 10])
def test_bound_items(bd):
    mx = (1 << bd) - 1
    tc, want = itc.checker(bd, False)                                         # flat prediction: the residual is +-half the range
    pred = itc.block(tc.pred0, int(tc.items[0]["pred_off"]), 64, 64, 64)
    rec = itc.block(want["rec"], int(tc.items[0]["rec_off"]), int(tc.items[0]["rec_stride"]), 64, 64)
    assert want["num_sig"][0] == 0 and want["abs_sum"][0] == 0 and np.array_equal(rec, pred)
    assert int(want["dist"][0]) == 2048 * (((mx + 1) // 2) ** 2 + (mx - (mx + 1) // 2) ** 2)
    tc, want = itc.checker(bd, True)                                          # the opposite checkerboard: +-the full range
    pred = itc.block(tc.pred0, int(tc.items[0]["pred_off"]), 64, 64, 64)
    rec = itc.block(want["rec"], int(tc.items[0]["rec_off"]), int(tc.items[0]["rec_stride"]), 64, 64)
    assert want["num_sig"][0] == 0 and np.array_equal(rec, pred) and int(want["dist"][0]) == 4096 * mx * mx
    assert (int(want["dist"][0]) > 1 << 31) == (bd == 10)
    tc, want = itc.bounds_case(bd)
    assert [int(v) for v in want["num_sig"][:4]] == [0, 1, 2, 3] and itc.EMT_SIG_NUM_THR == 2
    assert want["abs_sum"][4] == 0 and want["dist"][4] == 0
    for i in (5, 6):                                                          # quantised to zero by the QP, a non-zero residual: rec == pred
        it = tc.items[i]
        w = int(it["w"])
        assert want["num_sig"][i] == 0 and want["dist"][i] > 0
        assert np.array_equal(itc.block(want["rec"], int(it["rec_off"]), int(it["rec_stride"]), w, w), itc.block(tc.pred0, int(it["pred_off"]), int(it["pred_stride"]), w, w))


def entry(*a):
    return capi.lib().vvcgpu_intra_tu_code_batch(*a)


def test_argument_checks_without_device():
    one = C.c_void_p(16)                                                      # a non-null, aligned address that is never read: every check comes first
    #     refs preds org  pred rec  level tus  n  list flags bd  clp       abs  sig  dist mode stream
    ok = [one, one, one, one, one, one, one, 1, one, 3, 10, 0, 1023, one, one, one, one, None]
    assert entry(*(ok[:7] + [0] + ok[8:])) == 0                               # n == 0: a no-op, whatever else is passed
    assert entry(*[None if isinstance(v, C.c_void_p) else 0 if i == 7 else v for i, v in enumerate(ok)]) == 0

    def refused(changes, code=-1, word=None):
        a = list(ok)
        for i, v in changes.items():
            a[i] = v
        rc = entry(*a)
        text = capi.lib().vvcgpu_last_error().decode()
        assert rc == code and text.startswith("intra_tu_code_batch:"), (changes, rc, text)
        if word:
            assert word in text, text
    for i in (0, 1, 2, 4, 5, 6, 13, 14, 15, 16):                              # every required array
        refused({i: None}, word="null pointer")
    refused({3: None}, word="null pointer")                                   # pred_base under WRITE_PRED
    refused({7: -1})
    refused({9: 4}, word="flags")
    refused({9: -1}, word="flags")
    refused({11: 5, 12: 4}, word="clip range")
    refused({12: 32768}, word="clip range")
    refused({1: C.c_void_p(8)}, word="16-byte aligned")
    refused({6: C.c_void_p(24)}, word="16-byte aligned")
    refused({10: 12}, code=-3, word="bit depth")
    refused({10: 7}, code=-3, word="bit depth")
