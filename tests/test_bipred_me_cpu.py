"""CPU checks of the whole bi-predictive refinement (vvcgpu_bipred_me_batch): the tests' restatement of the loop of InterSearch::predInterSearch
(tests/bipred_me_cases.py) against the results the compiled reference's own xMotionEstimation / xCheckBestMVP / motionCompensation gave
(tests/golden/bipred_me.npz), and the host-side argument checks (no device is touched).  The structs' layout: tests/test_abi.py."""
import ctypes as C
import os

import numpy as np
import pytest

import bipred_me_cases as bc
import pu_search_kit as kit
from vvcsoftware_vtm_amd import abi, capi

G = os.path.join(os.path.dirname(__file__), "golden")
W, H = 256, 128


def _lib():
    if not os.path.exists(capi.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return capi.lib()


@pytest.mark.parametrize("bd", [10, 8])
def test_restatement_equals_reference_golden(bd):
    """every item of the fixture: result and trace of the restatement == what the reference's primitives gave under the generator's driving of the
    loop; no item trips the reference's CHECK; the fixture holds the cases the device tests rely on"""
    g = np.load(os.path.join(G, "bipred_me.npz"))
    k = "bd%d_" % bd
    items, want, want_trace = g[k + "items"], g[k + "want"], g[k + "trace"]
    assert len(items) >= 100 and int(g[k + "dropped"]) * 4 <= int(g[k + "generated"]) and len(items) + int(g[k + "dropped"]) == int(g[k + "generated"])
    planes = kit.pad(g[k + "planes"])
    assert planes.shape[1:] == (H + 2 * bc.MARGIN, W + 2 * bc.MARGIN)
    seen = set()
    for cfg, idx in bc.golden_groups(g, bd):
        s = bc.Searcher(g[k + "org"], planes, cfg)
        for i in idx:
            it = items[i]
            res, trace = s.search(it, strict=True, facts=seen)
            assert res.tobytes() == want[i].tobytes(), (i, res, want[i])
            assert np.array_equal(trace, want_trace[i]), (i, trace, want_trace[i])
            n = int(res["me_calls"])
            assert n >= 1 and trace[n:].tobytes() == bytes(trace[n:].nbytes)
            seen |= {("shape", int(it["w"]), int(it["h"])), ("n_ref", int(it["n_ref"][0])), ("n_ref", int(it["n_ref"][1])), ("range", cfg["search_range"]),
                     ("num_iter", cfg["num_iter"]), ("pick", cfg["pick_list_by_cost"]), ("mvd_l1_zero", cfg["mvd_l1_zero"]), ("clip_key", cfg["clip_key"]),
                     ("hadamard", cfg["use_hadamard"]), ("sub_shift", int(it["sub_shift"])), ("passes", kit.passes(trace, n)), ("closing", int(res["closing"]))}
            e = it["ref"][int(trace[0]["list"])][int(trace[0]["ref"])]["mv"]
            if abs(int(trace[0]["int_mv"][0]) * 4 - int(e[0])) > 2000:                      # a far-out entry vector that clipMv brought back
                seen.add(("corner", int(it["pos_x"]) == 0))
            blk = g[k + "org"][int(it["pos_y"]):int(it["pos_y"]) + int(it["h"]), int(it["pos_x"]):int(it["pos_x"]) + int(it["w"])]
            if blk.min() == blk.max():
                seen.add("flat")
    need = {("shape", w, h) for w in bc.SIDES for h in bc.SIDES} | {("n_ref", 1), ("n_ref", 2), ("n_ref", 4), ("range", 4), ("range", 2)}
    need |= {(f, v) for f in ("pick", "mvd_l1_zero", "clip_key", "hadamard", "sub_shift", "closing") for v in (0, 1)}
    need |= {("num_iter", 4), ("num_iter", 1), ("passes", 1), ("passes", 2), ("passes", 3), ("passes", 4), ("corner", True), ("corner", False)}
    need |= {"flat", "mvp_switch", "nonzero_ref_accepted", "closing_changes_bits"}
    assert need <= seen, need - seen


def test_the_check_of_the_reference_is_modelled():
    """strict mode raises where xCheckBestMVP's CHECK would: a predictor that is not the indexed candidate"""
    s = bc.Searcher(np.zeros((8, 8), np.int16), np.zeros((1, 8, 8), np.int16), bc.cfg_dict(10.0, 8, 8, 10))
    a = bc.ref_record(0, [0, 0], [[4, 4], [8, 8]], 0)
    assert s.check_best_mvp(a, [8, 8], [4, 4], 0, 20, 1000, strict=True) == ([8, 8], 1, 8, 880)      # a difference of 4 takes 7 bits, of 0 one bit: 2 x 6 bits saved at lambda 10
    with pytest.raises(bc.RefThrows):
        s.check_best_mvp(a, [8, 8], [5, 4], 0, 20, 1000, strict=True)
    assert s.check_best_mvp(bc.ref_record(0, [0, 0], [[4, 4]], 0), [8, 8], [4, 4], 0, 20, 1000, strict=True) == ([4, 4], 0, 20, 1000)


def _cfg(**kw):
    c = abi.BipredMeCfg()
    c.lambda_, c.n_planes, c.ref_stride, c.pic_w, c.pic_h, c.max_cu_w, c.max_cu_h = 30.0, 2, 544, 256, 128, 128, 128
    c.ref_planes[0] = c.ref_planes[1] = 4096
    c.bit_depth, c.clp_min, c.clp_max, c.num_iter, c.bipred_search_range = 10, 0, 1023, 4, 4
    c.mvp_idx_cost[:] = (1, 1, 0)
    for f, v in kw.items():
        setattr(c, f, v)
    return c


def test_argument_checks_need_no_device():
    lib = _lib()
    P = C.c_void_p(4096)                     # never dereferenced: every check below fails before device work
    call = lambda *a: lib.vvcgpu_bipred_me_batch(*a)
    assert call(None, None, 0, None, None, None, None) == 0                                          # n == 0: a no-op
    assert call(P, P, -1, C.byref(_cfg()), P, P, None) == -1 and b"bipred_me_batch" in lib.vvcgpu_last_error()
    for k in (0, 1, 3, 4):                                                                             # org, items, cfg, results (trace may be null)
        a = [P, P, 3, C.byref(_cfg()), P, None, None]
        a[k] = None
        assert call(*a) == -1 and b"bipred_me_batch: null" in lib.vvcgpu_last_error(), k
    c = _cfg()
    c.ref_planes[1] = None
    assert call(P, P, 3, C.byref(c), P, None, None) == -1 and b"bipred_me_batch: null" in lib.vvcgpu_last_error()
    for field, v, word in (("pic_w", 0, b"geometry"), ("pic_h", -4, b"geometry"), ("max_cu_w", 0, b"geometry"), ("max_cu_h", 0, b"geometry"),
                           ("ref_stride", 0, b"geometry"), ("n_planes", 0, b"n_planes"), ("n_planes", 17, b"n_planes"), ("clp_min", 1024, b"clip"),
                           ("lambda_", -1.0, b"lambda"), ("lambda_", float("nan"), b"lambda"), ("lambda_", 2.0 ** 20, b"lambda"),
                           ("bipred_search_range", 0, b"search_range"), ("bipred_search_range", 9, b"search_range"), ("num_iter", 2, b"num_iter"),
                           ("num_iter", 0, b"num_iter"), ("max_pu_w", 24, b"max_pu"), ("max_pu_h", 256, b"max_pu")):
        assert call(P, P, 3, C.byref(_cfg(**{field: v})), P, None, None) == -1, field
        assert b"bipred_me_batch" in lib.vvcgpu_last_error() and word in lib.vvcgpu_last_error(), (field, lib.vvcgpu_last_error())
    for bd in (7, 11):
        assert call(P, P, 3, C.byref(_cfg(bit_depth=bd)), P, None, None) == -3 and b"bit depth" in lib.vvcgpu_last_error()
