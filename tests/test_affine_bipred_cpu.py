"""CPU checks of the whole affine bi-predictive search (vvcgpu_affine_bipred_me_batch): the tests' restatement of the bi-predictive part of
InterSearch::xPredAffineInterSearch (tests/affine_bipred_cases.py) against the results the compiled reference's own xAffineMotionEstimation /
xCheckBestAffineMVP / motionCompensation gave (tests/golden/affine_bipred.npz), and the host-side argument checks (no device is
touched).  The structs' layout: tests/test_abi.py."""
import ctypes as C
import os

import numpy as np
import pytest

import affine_bipred_cases as ac
import pu_search_kit as kit
from vvcsoftware_vtm_amd import abi, capi

G = os.path.join(os.path.dirname(__file__), "golden")
W, H = 256, 128
SHAPES = [(16, 16), (32, 32), (64, 32), (32, 64), (128, 16), (16, 128), (128, 128)]


def _lib():
    if not os.path.exists(capi.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return capi.lib()


@pytest.mark.parametrize("bd", [10, 8])
def test_restatement_equals_reference_golden(bd):
    """every item of the fixture: result and trace of the restatement == what the reference's primitives gave under the generator's driving of the
    loop; the fixture holds the cases the device tests rely on"""
    g = np.load(os.path.join(G, "affine_bipred.npz"))
    k = "bd%d_" % bd
    items, want, want_trace = g[k + "items"], g[k + "want"], g[k + "trace"]
    assert len(items) >= 100
    planes = kit.pad(g[k + "planes"])
    assert planes.shape[1:] == (H + 2 * ac.MARGIN, W + 2 * ac.MARGIN)
    seen = set()
    groups = ac.golden_groups(g, bd)
    for cfg, idx in groups:
        s = ac.Searcher(g[k + "org"], planes, cfg)
        kinds = set()
        for i in idx:
            it = items[i]
            res, trace = s.search(it, facts=seen)
            assert res.tobytes() == want[i].tobytes(), (i, res, want[i])
            assert np.array_equal(trace, want_trace[i]), (i, trace, want_trace[i])
            n = int(res["me_calls"])
            assert n >= 1 and trace[n:].tobytes() == bytes(trace[n:].nbytes)
            six = int(it["six_param"])
            assert not six or min(int(v) for v in it["only_ref"]) >= 0                       # the 6-parameter items carry only_ref
            kinds.add(six)
            seen |= {("shape", int(it["w"]), int(it["h"])), ("n_ref", int(it["n_ref"][0]), int(it["n_ref"][1]), cfg["num_iter"], cfg["clip_key"]),
                     ("num_iter", cfg["num_iter"]), ("pick", cfg["num_iter"], cfg["pick_list_by_cost"]), ("mvd_l1_zero", cfg["num_iter"], cfg["mvd_l1_zero"]),
                     ("affine_type", cfg["affine_type"]), ("passes", kit.passes(trace, n)), ("closing", int(res["closing"]))}
            blk = g[k + "org"][int(it["pos_y"]):int(it["pos_y"]) + int(it["h"]), int(it["pos_x"]):int(it["pos_x"]) + int(it["w"])]
            if blk.min() == blk.max():
                assert (trace["steps"][:n] == 1).all()                                       # zero gradients: the singular system stops every search at once
                seen.add("flat")
        assert kinds == {0, 1}                                                               # 4- and 6-parameter items in every group
    need = {("shape",) + s for s in SHAPES} | {("n_ref", 2, 2, 4, 1), ("n_ref", 4, 1, 4, 0), ("pick", 1, 1), ("mvd_l1_zero", 1, 1), ("n_ref", 2, 4, 1, 1),
                                               ("affine_type", 0), ("affine_type", 1)}
    need |= {("passes", 2), ("passes", 3), ("passes", 4), ("closing", 0), ("closing", 1)}
    need |= {"flat", "mvp_switch", "nonzero_ref_accepted", "closing_changes_bits", "full_limit", "zero_delta_stop"}
    assert need <= seen, need - seen


def test_check_best_affine_mvp_by_hand():
    """the second-predictor rule: vectors 1 and 2 are coded against pred[i] + (mv[0] - pred[0]); a switch moves bits (uint32) and cost"""
    s = ac.Searcher(np.zeros((16, 16), np.int16), np.zeros((1, 16, 16), np.int16), ac.cfg_dict(10.0, 16, 16, 10))
    c0, c1 = [[16, 16], [16, 16], [16, 16]], [[32, 32], [40, 32], [32, 40]]
    a = ac.ref_record(0, c0, [c0, c1], 0)
    mv = [[32, 32], [40, 32], [32, 40]]
    # against c0: a difference of 4 quarter samples takes 7 bits, of 0 one bit: vector 0 (4, 4) 14 bits; vector 1 against c0[1] + (16, 16) = (32, 32):
    # (2, 0) 5 + 1 bits; vector 2 not counted for a 4-parameter PU.  against c1: 1 bit per component
    assert s.vec_bits(c0, 2, mv) == 20 and s.vec_bits(c1, 2, mv) == 4 and s.vec_bits(c0, 3, mv) == 26 and s.vec_bits(c1, 3, mv) == 6
    assert s.check_best_mvp(a, 2, mv, c0, 0, 30, 1000) == (c1, 1, 14, 840)
    assert s.check_best_mvp(a, 3, mv, c0, 0, 30, 1000) == (c1, 1, 10, 800)
    assert s.check_best_mvp(ac.ref_record(0, c0, [c0], 0), 2, mv, c0, 0, 30, 1000) == (c0, 0, 30, 1000)      # numCand < 2: nothing
    assert s.check_best_mvp(a, 2, mv, c0, 0, 3, 100) == (c1, 1, (3 - 21 + 5) & 0xFFFFFFFF, (100 - 30 + int(10.0 * ((3 - 21 + 5) & 0xFFFFFFFF))) & kit.U64_MAX)


def _cfg(**kw):
    c = abi.AffineBipredCfg()
    c.lambda_, c.n_planes, c.ref_stride, c.pic_w, c.pic_h, c.max_cu_w, c.max_cu_h = 30.0, 2, 544, 256, 128, 128, 128
    c.ref_planes[0] = c.ref_planes[1] = 4096
    c.bit_depth, c.clp_min, c.clp_max, c.num_iter, c.affine_type = 10, 0, 1023, 4, 1
    c.mvp_idx_cost[:] = (1, 1, 0)
    for f, v in kw.items():
        setattr(c, f, v)
    return c


def test_argument_checks_need_no_device():
    lib = _lib()
    P = C.c_void_p(4096)                     # never dereferenced: every check below fails before device work
    call = lambda *a: lib.vvcgpu_affine_bipred_me_batch(*a)
    assert call(None, None, 0, None, None, None, None) == 0                                          # n == 0: a no-op
    assert call(P, P, -1, C.byref(_cfg()), P, P, None) == -1 and b"affine_bipred_me_batch" in lib.vvcgpu_last_error()
    for k in (0, 1, 3, 4):                                                                             # org, items, cfg, results (trace may be null)
        a = [P, P, 3, C.byref(_cfg()), P, None, None]
        a[k] = None
        assert call(*a) == -1 and b"affine_bipred_me_batch: null" in lib.vvcgpu_last_error(), k
    c = _cfg()
    c.ref_planes[1] = None
    assert call(P, P, 3, C.byref(c), P, None, None) == -1 and b"affine_bipred_me_batch: null" in lib.vvcgpu_last_error()
    for field, v, word in (("pic_w", 0, b"geometry"), ("pic_h", -4, b"geometry"), ("max_cu_w", 0, b"geometry"), ("max_cu_h", 0, b"geometry"),
                           ("ref_stride", 0, b"geometry"), ("n_planes", 0, b"n_planes"), ("n_planes", 17, b"n_planes"), ("clp_min", 1024, b"clip"),
                           ("lambda_", -1.0, b"lambda"), ("lambda_", float("nan"), b"lambda"), ("lambda_", 2.0 ** 20, b"lambda"),
                           ("num_iter", 2, b"num_iter"), ("num_iter", 0, b"num_iter"), ("max_pu_w", 24, b"max_pu"), ("max_pu_w", 8, b"max_pu"),
                           ("max_pu_h", 256, b"max_pu")):
        assert call(P, P, 3, C.byref(_cfg(**{field: v})), P, None, None) == -1, field
        assert b"affine_bipred_me_batch" in lib.vvcgpu_last_error() and word in lib.vvcgpu_last_error(), (field, lib.vvcgpu_last_error())
    for bd in (7, 11):
        assert call(P, P, 3, C.byref(_cfg(bit_depth=bd)), P, None, None) == -3 and b"bit depth" in lib.vvcgpu_last_error()
