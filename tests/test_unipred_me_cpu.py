"""CPU checks of the uni-predictive stage (vvcgpu_unipred_me_batch): the tests' restatement of the uni-predictive loop of InterSearch::predInterSearch
(tests/unipred_me_cases.py) against the results the compiled reference's own xEstimateMvPredAMVP / xMotionEstimation / xCheckBestMVP gave
(tests/golden/unipred_me.npz), the exported symbol, and the host-side argument checks (no device is touched).  The structs' layout:
tests/test_abi.py."""
import ctypes as C
import os

import numpy as np
import pytest

import unipred_me_cases as uc
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
    """every item of the fixture: result and out-item of the restatement == what the reference's primitives gave under the generator's driving of the
    loop; the fixture holds the cases the issue lists"""
    g = np.load(os.path.join(G, "unipred_me.npz"))
    k = "bd%d_" % bd
    items, want, want_out = g[k + "items"], g[k + "want"], g[k + "out"]
    assert len(items) >= 100 and int(g[k + "dropped"]) * 4 <= int(g[k + "generated"]) and len(items) + int(g[k + "dropped"]) == int(g[k + "generated"])
    planes = kit.pad(g[k + "planes"])
    assert planes.shape[1:] == (H + 2 * uc.MARGIN, W + 2 * uc.MARGIN)
    seen = set()
    for cfg, idx in uc.golden_groups(g, bd):
        s = uc.Searcher(g[k + "org"], planes, cfg)
        for i in idx:
            it = items[i]
            f = set()
            res, out = s.search(it, facts=f)
            assert res.tobytes() == want[i].tobytes(), (i, res, want[i])
            assert out.tobytes() == want_out[i].tobytes(), (i, out, want_out[i])
            seen |= f | uc.golden_facts(g[k + "org"], cfg, it, f)
    assert uc.GOLDEN_NEED <= seen, uc.GOLDEN_NEED - seen


def test_the_cached_start_path_takes_the_fast_settings_from_the_cached_vector():
    """the restatement's cached-start path (:1759-1766) is orc_tz_search with the fast settings, started at the cached vector, no 2Nx2N predictor"""
    org, planes, cfg, items = uc.fresh_set(11, 10, [(16, 16)] * 6, n_ref=(1, 0), search_range=32, ext=True)
    s = uc.Searcher(org, planes, cfg)
    differ = 0
    for it in items:
        n = it.copy()
        n["ref"][0][0]["flags"] = 0
        a = n.copy()
        a["ref"][0][0]["flags"] = abi.UNIPRED_CACHED | abi.UNIPRED_PRED2
        a["ref"][0][0]["cached_mv"] = (5, -3)
        b = a.copy()
        b["ref"][0][0]["pred2"] = (40, 40)                        # ignored on the cached path
        b["tz_flags"] = 0                                         # so are the extended settings
        st = np.zeros((2, 3), np.uint64)                          # probes, rounds, raster probes of the one TZ search of a call
        ra, rb = s.search(a)[0], s.search(b)[0]
        s.o.orc_tz_stats(uc.p(st[0]))
        rn = s.search(n)[0]
        s.o.orc_tz_stats(uc.p(st[1]))
        assert ra.tobytes() == rb.tobytes()
        assert ra["s"][0][0]["tmpl_cost"].tolist() == rn["s"][0][0]["tmpl_cost"].tolist()      # the predictor choice does not depend on the path
        differ += int(st[0][0]) < int(st[1][0])                   # the extended settings always run a raster, the fast ones stop early
    assert differ == len(items)


def test_the_entry_is_exported_and_declared():
    lib = _lib()
    assert "vvcgpu_unipred_me_batch" in capi.declared_symbols() and hasattr(lib, "vvcgpu_unipred_me_batch")
    restype, argtypes = capi.prototypes()["vvcgpu_unipred_me_batch"]
    assert restype is C.c_int and argtypes == (C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)


def _cfg(**kw):
    c = abi.UnipredMeCfg()
    c.lambda_, c.n_planes, c.ref_stride, c.pic_w, c.pic_h, c.max_cu_w, c.max_cu_h = 30.0, 2, 544, 256, 128, 128, 128
    c.ref_planes[0] = c.ref_planes[1] = 4096
    c.bit_depth, c.clp_min, c.clp_max = 10, 0, 1023
    c.n_ref[:] = (2, 2)
    for l in range(2):
        for r in range(4):
            c.ref_plane[l][r], c.search_range[l][r] = r & 1, 32
    c.list1_to_list0[:] = (-1, 0, -1, -1)
    c.mvp_idx_cost[:] = (1, 1, 0)
    for f, v in kw.items():
        if isinstance(v, tuple) and f in ("ref_plane", "search_range"):
            getattr(c, f)[v[0]][v[1]] = v[2]
        elif isinstance(v, tuple):
            getattr(c, f)[v[0]] = v[1]
        else:
            setattr(c, f, v)
    return c


def test_argument_checks_need_no_device():
    lib = _lib()
    P = C.c_void_p(4096)                     # never dereferenced: every check below fails before device work
    call = lambda *a: lib.vvcgpu_unipred_me_batch(*a)
    assert call(None, None, 0, None, None, None, None) == 0                                          # n == 0: a no-op
    assert call(P, P, -1, C.byref(_cfg()), P, P, None) == -1 and b"unipred_me_batch" in lib.vvcgpu_last_error()
    for k in (0, 1, 3, 4):                                                                             # org, items, cfg, results (the out-items may be null)
        a = [P, P, 3, C.byref(_cfg()), P, None, None]
        a[k] = None
        assert call(*a) == -1 and b"unipred_me_batch: null" in lib.vvcgpu_last_error(), k
    c = _cfg()
    c.ref_planes[1] = None
    assert call(P, P, 3, C.byref(c), P, None, None) == -1 and b"unipred_me_batch: null" in lib.vvcgpu_last_error()
    for field, v, word in (("pic_w", 0, b"geometry"), ("pic_h", -4, b"geometry"), ("max_cu_w", 0, b"geometry"), ("max_cu_h", 0, b"geometry"),
                           ("ref_stride", 0, b"geometry"), ("n_planes", 0, b"n_planes"), ("n_planes", 17, b"n_planes"), ("clp_min", 1024, b"clip"),
                           ("lambda_", -1.0, b"lambda"), ("lambda_", float("nan"), b"lambda"), ("lambda_", 2.0 ** 20, b"lambda"),
                           ("n_ref", (0, 0), b"n_ref"), ("n_ref", (0, 5), b"n_ref"), ("n_ref", (1, -1), b"n_ref"), ("n_ref", (1, 5), b"n_ref"),
                           ("ref_plane", (0, 1, 2), b"ref_plane"), ("ref_plane", (1, 0, -1), b"ref_plane"), ("search_range", (0, 0, 0), b"search_range"),
                           ("search_range", (1, 1, 257), b"search_range"), ("list1_to_list0", (0, 2), b"list1_to_list0"),
                           ("list1_to_list0", (1, -2), b"list1_to_list0"), ("max_pu_w", 24, b"max_pu"), ("max_pu_h", 256, b"max_pu")):
        assert call(P, P, 3, C.byref(_cfg(**{field: v})), P, None, None) == -1, field
        assert b"unipred_me_batch" in lib.vvcgpu_last_error() and word in lib.vvcgpu_last_error(), (field, lib.vvcgpu_last_error())
    for bd in (7, 11):
        assert call(P, P, 3, C.byref(_cfg(bit_depth=bd)), P, None, None) == -3 and b"bit depth" in lib.vvcgpu_last_error()
