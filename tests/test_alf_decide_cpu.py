"""CPU side of vvcgpu_alf_frame_stats / vvcgpu_alf_ctu_dist: the restatement the device tests compare with (tests/alf_decide_cases.py) reproduces
every result of the compiled reference stored in tests/golden/alf_decide.npz, bit for bit; the fixture still holds the cases the tests rely on --
above all, its large-magnitude records tell three wrong summation orders from the reference's; the entries' argument checks work without a device;
header, bindings and library agree on the two names."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import alf_decide_cases as adc
from vvcsoftware_vtm_amd import capi

CASES = adc.load_golden()


@pytest.mark.parametrize("c", CASES, ids=[c["id"] for c in CASES])
def test_restatement_reproduces_the_reference(c):
    rec = adc.case_records(c)
    assert rec.shape == (c["n_ctu"], c["n_cls"], adc.n_vals(adc.N_OF[c["filter_type"]])) and int(np.abs(rec).max()) < 1 << 53
    assert np.array_equal(adc.frame_stats(rec, c["enable"]), c["frame"])
    got = adc.bits(adc.ctu_dist(rec, c["coeff"], c["idx"], c["coeff_bits"]))
    want = adc.bits(c["dist"])
    assert np.array_equal(got, want), "CTUs %s differ" % np.nonzero((got != want).any(1))[0].tolist()


def test_fixture_holds_the_cases_the_tests_rely_on():
    """both shapes, 25 classes and 1, shared and all-zero filters, negative y, the three kinds of mask, coeff_bits 10 and another value -- and on every
    case of the large set each wrong order (reversed classes, pairwise tree over the classes, pairwise tree inside the row sums) changes the
    reference's result for at least one CTU in four"""
    adc.check_fixture(CASES, adc.wrong_orders_restated)
    assert {c["kind"] for c in CASES} == {adc.REAL, adc.NOISE, adc.LARGE}


def test_sums_below_2_53_equal_the_reference_double_accumulation():
    """the precondition stated in vvcgpu.h, on the fixture: adding the records as doubles in CTU order (what getFrameStat does) gives the int64 sums"""
    for c in CASES:
        rec = adc.case_records(c).astype(np.float64)
        acc = np.zeros(rec.shape[1:], np.float64)
        for i in np.nonzero(c["enable"])[0]:
            acc = acc + rec[i]
        assert np.array_equal(acc, c["frame"].astype(np.float64)) and np.array_equal(acc.astype(np.int64), c["frame"]), c["id"]


# ---- the entries' argument checks: all before any device work -----------------------------------------------------------------------------------------
P = C.c_void_p(64)          # a non-null "device" address that is never touched


def frame_stats(ctu_stats=P, n_ctu=3, n_classes=25, n_vals=183, enable=None, accumulate=0, frame_out=P):
    return capi.lib().vvcgpu_alf_frame_stats(ctu_stats, n_ctu, n_classes, n_vals, enable, accumulate, frame_out, None)


def ctu_dist(ctu_stats=P, n_ctu=3, n_classes=25, filter_type=1, coeff=True, n_filters=3, idx=True, coeff_bits=10, dist_out=P):
    N = 13 if filter_type == 1 else 7
    cs = np.zeros((25, N), np.int32)
    fi = (np.arange(25) % max(1, min(n_filters, 25))).astype(np.int16) if idx is True else idx
    return capi.lib().vvcgpu_alf_ctu_dist(ctu_stats, n_ctu, n_classes, filter_type, C.c_void_p(cs.ctypes.data) if coeff else None, n_filters,
                                          None if fi is None else C.c_void_p(fi.ctypes.data), coeff_bits, dist_out, None)


def refused(rc, name):
    assert rc == -1, rc
    assert name.encode() in capi.lib().vvcgpu_last_error(), capi.lib().vvcgpu_last_error()


def test_frame_stats_argument_checks():
    assert frame_stats(n_ctu=0) == 0
    assert frame_stats(n_ctu=0, n_classes=1, n_vals=57, accumulate=1) == 0
    for kw in (dict(ctu_stats=None), dict(frame_out=None), dict(n_ctu=-1), dict(n_classes=0), dict(n_classes=2), dict(n_classes=24), dict(n_classes=26),
               dict(n_vals=0), dict(n_vals=56), dict(n_vals=182), dict(n_vals=184), dict(n_ctu=0, n_classes=3), dict(n_ctu=0, n_vals=13)):
        refused(frame_stats(**kw), "alf_frame_stats")


def test_ctu_dist_argument_checks():
    assert ctu_dist(n_ctu=0) == 0
    assert ctu_dist(n_ctu=0, n_classes=1, filter_type=0, n_filters=1, idx=None) == 0
    bad_idx = np.arange(25, dtype=np.int16) % 3
    bad_idx[17] = 3
    neg_idx = np.zeros(25, np.int16)
    neg_idx[24] = -1
    for kw in (dict(ctu_stats=None), dict(dist_out=None), dict(coeff=False), dict(idx=None), dict(n_ctu=-1), dict(n_classes=0), dict(n_classes=24),
               dict(filter_type=-1), dict(filter_type=2), dict(n_filters=0), dict(n_filters=26), dict(n_filters=-3), dict(idx=bad_idx), dict(idx=neg_idx),
               dict(coeff_bits=1), dict(coeff_bits=17), dict(coeff_bits=0), dict(n_ctu=0, coeff_bits=17), dict(n_ctu=0, idx=bad_idx)):
        refused(ctu_dist(**kw), "alf_ctu_dist")
    refused(ctu_dist(idx=bad_idx), "filter index 3 of class 17")


def test_header_bindings_and_library_agree():
    names = ["vvcgpu_alf_frame_stats", "vvcgpu_alf_ctu_dist"]
    protos = capi.prototypes()
    assert set(names) <= set(capi.declared_symbols())
    v, i = C.c_void_p, C.c_int
    assert protos[names[0]] == (i, (v, i, i, i, v, i, v, v))
    assert protos[names[1]] == (i, (v, i, i, i, v, i, v, i, v, v))
    exported = subprocess.check_output(["nm", "-D", "--defined-only", capi.LIB_PATH], text=True).split()
    for n in names:
        assert n in exported and hasattr(capi.lib(), n)
