"""CPU checks of explicit weighted prediction (vvcgpu_mc_wp_batch): the host-side argument checks (no device is touched) and the tests' restatement of
the weighted epilogue against the reference's own addWeightUni / addWeightBi (tests/golden/wp.npz).  The table entry's layout: tests/test_abi.py."""
import ctypes as C
import os

import numpy as np

import wp_cases
from oraclelib import oracle
from vvcsoftware_vtm_amd import capi

G = os.path.join(os.path.dirname(__file__), "golden")


def _lib():
    if not os.path.exists(capi.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return capi.lib()


def test_wp_argument_checks_need_no_device():
    lib = _lib()
    P = C.c_void_p(4096)                     # never dereferenced: every check below fails before device work
    call = lambda *a: lib.vvcgpu_mc_wp_batch(*a)
    assert call(None, None, None, None, 0, None, 0, 10, 0, 1023, None) == 0                         # n == 0: a no-op
    assert call(P, P, P, P, -1, P, 1, 10, 0, 1023, None) == -1
    for k in (0, 2, 3, 5):                                                                            # ref0, dst, descs, wp
        a = [P, P, P, P, 4, P, 1, 10, 0, 1023, None]
        a[k] = None
        assert call(*a) == -1 and b"mc_wp_batch" in lib.vvcgpu_last_error(), k
    for nwp in (0, -1, 32768):
        assert call(P, P, P, P, 4, P, nwp, 10, 0, 1023, None) == -1 and b"n_wp" in lib.vvcgpu_last_error()
    assert call(P, P, P, C.c_void_p(4096 + 8), 4, P, 1, 10, 0, 1023, None) == -1 and b"aligned" in lib.vvcgpu_last_error()
    assert call(P, P, P, P, 4, C.c_void_p(4096 + 4), 1, 10, 0, 1023, None) == -1 and b"aligned" in lib.vvcgpu_last_error()
    for bd in (7, 11, 12):
        assert call(P, P, P, P, 4, P, 1, bd, 0, 1023, None) == -3 and b"bit depth" in lib.vvcgpu_last_error()


def test_wp_param_helper_restates_get_wp_scaling():
    from vvcsoftware_vtm_amd import ops
    assert ops.wp_param(10, 5, 40, -7) == (40, 0, -28, 5)                      # uni: offset << (bd - 8), shift = log2 denominator
    assert ops.wp_param(8, 5, 40, -7, 20, 3) == (40, 20, -4, 6)                 # bi: o0 + o1, shift + 1
    assert ops.wp_param(10, 0, 1, 3, 1, 4, high_precision_offsets=True) == (1, 1, 7, 1)


def test_wp_restatement_equals_reference_golden():
    """the restatement of tests/wp_cases.py on the CPU restatement's bi = 2 intermediates == the reference's addWeightUni / addWeightBi on the
    reference's own intermediates"""
    g = np.load(os.path.join(G, "wp.npz"))
    for bd in (8, 10):
        k = "bd%d_" % bd
        d, wp, want = g[k + "descs"], g[k + "wp"], g[k + "want"]
        assert len(d) >= 80 and set(np.unique(d["bi"])) == {0, 1} and set(np.unique(d["is_luma"])) == {0, 1}
        got = wp_cases.expected(oracle().orc_mc_batch, g[k + "r0"], g[k + "r1"], d, wp, bd, 0, (1 << bd) - 1, np.full(want.size, -5, np.int16))
        assert np.array_equal(got, want), bd
        assert (want == 0).any() and (want == (1 << bd) - 1).any()                 # outputs clip at both ends
