"""CPU: which decisions of the deblocking filters the inputs of tests/cases.py::deblock_census_cases reach.  orc_deblock_census (oracle/restate/deblock.cpp)
is orc_deblock with a counter per event and edge direction; the device tests (tests/test_gpu_deblock_census.py) compare the kernels with the restatement on
the same inputs, so an event counted here is a branch on which a kernel that takes it differently fails there.  The thresholds are conditions on the
INPUTS: the restatement alone decides them."""
import ctypes as C

import numpy as np

import cases
from oraclelib import oracle, p

MIN_EQ, MIN_REST = 8, 64          # per direction (chroma: per plane and direction): events of a value exactly on / one below its threshold; the rest


def census_names():
    txt = C.c_char_p()
    n = oracle().orc_deblock_census_names(C.byref(txt))
    names = txt.value.decode().rstrip(",").split(",")
    assert len(names) == n
    return names


def census_add(counters, w, h, Y, Cb, Cr, ev, eh, qpl, qpc, cfg):
    """counters (2, n) int64 += the events of one picture; -> the filtered planes"""
    Y, Cb, Cr = Y.copy(), Cb.copy(), Cr.copy()
    rc = oracle().orc_deblock_census(p(Y), w, p(Cb), p(Cr), w // 2, w, h, p(ev), p(eh), p(qpl), p(qpc), C.byref(cfg), p(counters))
    assert rc == 0
    return Y, Cb, Cr


def census_of_cases(cs):
    cn = np.zeros((2, len(census_names())), np.int64)
    for c in cs:
        census_add(cn, c["w"], c["h"], c["Y"], c["Cb"], c["Cr"], c["ev"], c["eh"], c["qpl"], c["qpc"], cases.deblock_cfg_struct(c["cfg"]))
    return cn


def test_census_changes_nothing():
    """one statement of the arithmetic: the counting pass leaves the planes orc_deblock leaves"""
    for c in cases.deblock_census_cases()[::7]:
        cfg = cases.deblock_cfg_struct(c["cfg"])
        want = [c[k].copy() for k in ("Y", "Cb", "Cr")]
        oracle().orc_deblock(p(want[0]), c["w"], p(want[1]), p(want[2]), c["w"] // 2, c["w"], c["h"], p(c["ev"]), p(c["eh"]), p(c["qpl"]), p(c["qpc"]), C.byref(cfg))
        got = census_add(np.zeros((2, len(census_names())), np.int64), c["w"], c["h"], c["Y"], c["Cb"], c["Cr"], c["ev"], c["eh"], c["qpl"], c["qpc"], cfg)
        assert all(np.array_equal(g, w_) for g, w_ in zip(got, want))


def test_census_names():
    names = census_names()
    assert len(set(names)) == len(names) == 38 + 2 * 8
    for want in ("seg", "d_eq_beta_m1", "dm_eq_thr", "delta_eq_thr_m1", "strong_clip_q2", "strong_outside_clp", "tc_idx_hi", "beta_idx_lo", "cb_qp_ge70", "cr_qp_lt0"):
        assert want in names


def test_configurations_cover_the_issue():
    rows = cases.DBK_CFGS
    assert {r[0] for r in rows} == {8, 9, 10} and (10, 8) in {(r[0], r[1]) for r in rows}
    assert {(6, -6), (-6, 6)} <= {(r[2], r[3]) for r in rows}
    assert {12, -12} <= {r[4] for r in rows} and {12, -12} <= {r[5] for r in rows}
    narrow = cases.deblock_cfg_dict(*[r for r in rows if r[6]][0])
    assert len(set(zip(narrow["clp_min"], narrow["clp_max"]))) == 3 and min(narrow["clp_min"]) > 0
    cs = cases.deblock_census_cases()
    for k in ("qpl", "qpc"):
        q = np.concatenate([c[k].ravel() for c in cs])
        assert q.min() == -12 and q.max() == 63
    # every BS / flag combination deblock_maps(..., 'random') allows: luma BS 0..2, chroma BS 0..2, both flags
    allowed = {b for b in range(64) if (b & 3) != 3 and ((b >> 2) & 3) != 3}
    assert allowed <= set(np.concatenate([c["ev"].ravel() for c in cs]).tolist()) and allowed <= set(np.concatenate([c["eh"].ravel() for c in cs]).tolist())
    assert {(c["w"], c["h"]) for c in cs} == {(136, 72), (200, 120), (8, 8), (16, 8), (8, 16), (520, 24)}


def test_new_inputs_reach_every_event():
    names = census_names()
    cn = census_of_cases(cases.deblock_census_cases())
    short = ["%s %s: %d < %d" % ("ver hor".split()[d], n, cn[d, i], MIN_EQ if "_eq_" in n else MIN_REST)
             for d in range(2) for i, n in enumerate(names) if cn[d, i] < (MIN_EQ if "_eq_" in n else MIN_REST)]
    assert not short, "\n".join(short)


def _filtered(c):
    return census_add(np.zeros((2, len(census_names())), np.int64), c["w"], c["h"], c["Y"], c["Cb"], c["Cr"], c["ev"], c["eh"], c["qpl"], c["qpc"],
                      cases.deblock_cfg_struct(c["cfg"]))


def test_no_interior_edge():
    """8 x 8 has no edge inside the picture: with every map byte set the planes come back as they went in"""
    c = [c for c in cases.deblock_census_cases() if (c["w"], c["h"]) == (8, 8)][0]
    assert c["ev"].all() and c["eh"].all()
    assert all(np.array_equal(got, c[k]) for got, k in zip(_filtered(c), ("Y", "Cb", "Cr")))


def test_wild_samples_are_filtered():
    """the wild cases hold samples at both ends of int16, and the restatement filters lines that hold them"""
    ws = [c for c in cases.deblock_census_cases() if c["name"].startswith("wild")]
    assert len(ws) == 2
    for c in ws:
        Y, mx = c["Y"], (1 << c["cfg"]["bd_luma"]) - 1
        assert Y.max() == 32767 and Y.min() == -32768
        assert (((Y < 0) | (Y > mx)) & (_filtered(c)[0] != Y)).sum() >= 64
