"""Generates tests/golden/intra_mode_cand.npz: intra mode pre-selection passes (IntraSearch::estIntraPredLumaQT, IntraSearch.cpp:405-522 and 591-618)
whose every pixel step and list step is the COMPILED REFERENCE's.  Build machine only (needs the reference tree and oracle/_ref/libvtmref.so, i.e. a
build() where the reference exists):
    python tests/golden/gen_intra_mode_cand.py

estIntraPredLumaQT itself needs a CodingStructure with its buffers, the CABAC estimator and the mode control around it; so
gen_intra_mode_cand_driver.cpp -- compiled here against the reference's headers (the include set of oracle/Makefile's CXXFLAGS_REF,
-fno-access-control) and linked with libvtmref.so -- exposes the reference's own useFilteredIntraRefSamples, xFilterReferenceSamples (as
initIntraPatternChType calls it), predIntraAng, RdCost::setDistParam(.., bUseHadamard) + distFunc, the cost expression of :436 and updateCandList, and
ref_pass() below drives them with the loops of :405-522 and :591-618, written here from the reference's text.  The tests' restatement
(tests/intra_mode_cand_cases.py) has its own writing of those loops over the CPU restatement's pixel steps; the generator asserts that it reproduces
every stored value.  Nothing of the reference is copied; only the data is stored.

Inputs of the cases, not results of the reference: the MPMs (PU::getIntraMPMs walks the coding structure), the four bit values (xFracModeBitsIntra needs
the CABAC state), interHad, numModesForFullRD, and the packed references -- the availability walk and xFillReferenceSamples need the coding structure;
the references are gathered by the CPU restatement's orc_intra_fill_refs, which tests/golden/intra_fill.npz checks against the reference's own calls."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

import intra_mode_cand_cases as imc  # noqa: E402
from oraclelib import p  # noqa: E402

REF = os.environ.get("REF", "/root/reference")
NUM_LUMA_MODE, DC_IDX = 67, 1
# per bit depth: flags, sqrt_lambda, the specs of intra_mode_cand_cases.make_case
SETS = {10: dict(flags=imc.USE_MPM, lam=27.375, specs=[
            (4, 4, dict(avail=0, gate="off")), (8, 8, dict(avail=3, gate=1)), (16, 16, dict(avail=0, gate=2)), (32, 32, dict(avail=4, gate="uncut")),
            (64, 64, dict(avail=0, gate=0)), (4, 8, dict(avail=3)), (8, 4, dict(avail=1, gate=1)), (4, 64, dict(avail=0, gate=2)), (64, 4, dict(avail=3)),
            (16, 4, dict(avail=2)), (8, 32, dict(avail=0, num_modes=5)), (32, 8, dict(avail=4, num_modes=8, gate="uncut")), (64, 16, dict(avail=0)),
            (16, 64, dict(avail=3, gate=1)), (32, 64, dict(avail=0, gate=2)), (64, 32, dict(avail=4)), (16, 16, dict(paint=33, gate="off")),
            (8, 8, dict(paint=2)), (8, 8, dict(paint=66, gate=1)), (4, 4, dict(paint=45)), (32, 16, dict(paint=2, gate=2)), (16, 32, dict(paint=66)),
            (16, 16, dict(flat=True, mpm=[3, 66, 1])), (4, 8, dict(flat=True, mpm=[0, 50, 18], gate="uncut")), (64, 64, dict(flat=True, mpm=[1, 2, 21])),
            (8, 16, dict(avail=3, num_modes=1)), (16, 8, dict(avail=0, gate=0)), (32, 32, dict(paint=21, num_modes=4)), (4, 16, dict(avail=4, gate=1)),
            (64, 8, dict(avail=0, gate=2))]),
        8: dict(flags=imc.USE_MPM, lam=8.5, specs=[
            (4, 4, dict(avail=3, gate=1)), (8, 8, dict(avail=0, gate=2)), (16, 16, dict(avail=4, gate=0)), (32, 32, dict(avail=0)),
            (64, 64, dict(avail=3, gate="uncut")), (4, 8, dict(avail=0, gate=2)), (8, 4, dict(avail=4)), (4, 64, dict(avail=3, gate=1)),
            (64, 4, dict(avail=0, gate=2)), (4, 32, dict(avail=1)), (32, 4, dict(avail=0, num_modes=6)), (8, 64, dict(avail=4, num_modes=2)),
            (64, 8, dict(avail=2)), (16, 32, dict(avail=0, gate=1)), (32, 16, dict(avail=3, gate=2)), (8, 16, dict(avail=0)), (16, 8, dict(paint=33)),
            (4, 4, dict(paint=2, gate="off")), (16, 16, dict(paint=66, gate=1)), (8, 4, dict(paint=11)), (4, 8, dict(paint=57, gate=2)),
            (64, 32, dict(paint=2)), (8, 8, dict(flat=True, mpm=[3, 66, 1], gate="uncut")), (32, 8, dict(flat=True, mpm=[0, 50, 18])),
            (4, 4, dict(flat=True, mpm=[5, 7, 9])), (32, 64, dict(avail=3, num_modes=7)), (16, 4, dict(avail=0, gate=0)), (16, 64, dict(paint=45, num_modes=3)),
            (64, 16, dict(avail=4, gate=1)), (8, 32, dict(avail=0, gate=2))])}


def driver():
    src = os.path.join(REF, "source", "Lib")
    inc = ["-I" + os.path.join(src, d) for d in ("", "CommonLib", "CommonLib/x86", "libmd5", "EncoderLib", "DecoderLib", "Utilities")]
    refdir = os.path.join(ROOT, "oracle", "_ref")
    out = os.path.join(tempfile.mkdtemp(), "libimref.so")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-fPIC", "-shared", "-msse4.1", "-w", "-DNDEBUG", "-fno-access-control"] + inc +
                          [os.path.join(HERE, "gen_intra_mode_cand_driver.cpp"), "-o", out, "-L" + refdir, "-lvtmref", "-Wl,-rpath," + refdir])
    D = C.CDLL(out)
    D.imref_dist.restype = C.c_uint64
    D.imref_cost.restype = C.c_double
    return D


class RefLists:
    """uiRdModeList / CandCostList and uiHadModeList / CandHadList, updated by the reference's updateCandList"""
    def __init__(self, D):
        self.D = D
        self.m = [np.zeros(NUM_LUMA_MODE, np.uint32) for _ in range(2)]
        self.c = [np.zeros(NUM_LUMA_MODE, np.float64) for _ in range(2)]
        self.n = [C.c_int(0), C.c_int(0)]

    def update(self, which, mode, cost, fast_num):
        assert self.D.imref_update_cand_list(mode, C.c_double(cost), p(self.m[which]), p(self.c[which]), C.byref(self.n[which]), fast_num) >= 0

    def modes(self, which):
        return [int(v) for v in self.m[which][:self.n[which].value]]

    def costs(self, which):
        return [float(v) for v in self.c[which][:self.n[which].value]]


def ref_pass(D, case, flags, lam):
    """:405-522 and :591-618 over the driver's primitives -> (satd [n][67], lists [n][16], costs [n][12])"""
    n = len(case.pus)
    satd = np.full((n, NUM_LUMA_MODE), imc.U64_MAX, np.uint64)
    lists, costs = np.full((n, 16), -1, np.int32), np.full((n, 12), np.inf)
    mx = (1 << case.bd) - 1
    D.imref_open(case.bd, 1 if flags & imc.NO_SMOOTHING else 0)
    for q, u in enumerate(case.pus):
        w, h, num = int(u["w"]), int(u["h"]), int(u["num_modes"])
        assert D.imref_load(p(case.refs_of(q)), w, h, 0, mx) == (0 if flags & imc.NO_SMOOTHING else 1)
        org = C.c_void_p(case.org.ctypes.data + 2 * (int(u["y"]) * imc.W + int(u["x"])))
        pred = np.zeros((h, w), np.int16)
        L = RefLists(D)
        checked = [False] * NUM_LUMA_MODE

        def evaluate(mode, rd_num):
            assert D.imref_pred(mode, D.imref_use_filtered(mode), p(pred)) == 0
            sad = D.imref_dist(org, imc.W, p(pred), w, w, h)
            satd[q][mode] = sad
            cost = D.imref_cost(C.c_uint64(sad), C.c_uint64(imc.mode_bits(mode, u["mpm"], u["bits"])), C.c_double(lam))
            L.update(0, mode, cost, rd_num)
            L.update(1, mode, float(sad), 3)
            checked[mode] = True
        for mode in range(NUM_LUMA_MODE):                                    # :405-446
            if mode > DC_IDX and (mode & 1):
                continue
            evaluate(mode, num)
        assert L.n[0].value == num                                          # :450 resizes to numModesForFullRD
        for parent in L.modes(0):                                            # :452-496, over a copy of the list
            if DC_IDX + 1 < parent < NUM_LUMA_MODE - 1:
                for sub in (-1, 1):
                    if not checked[parent + sub]:
                        evaluate(parent + sub, num)
        rd = L.modes(0)
        if flags & imc.USE_MPM:                                              # :499-522
            for j in range(3):
                if int(u["mpm"][j]) not in rd:
                    rd.append(int(u["mpm"][j]))
        had_m, had_c = L.modes(1), L.costs(1)
        final = len(rd)
        if int(u["inter_had"]) != imc.U64_MAX:                               # :591-618, the gate's condition being the caller's
            thr = float(int(u["inter_had"])) * imc.PBINTRA_RATIO
            if len(had_c) < 3 or had_c[2] > thr:
                final = min(final, 2)
            if len(had_c) < 2 or had_c[1] > thr:
                final = min(final, 1)
            if len(had_c) < 1 or had_c[0] > thr:
                final = 0
        lists[q][0], lists[q][1] = final, len(had_m)
        lists[q][2:2 + len(had_m)] = had_m
        lists[q][5:5 + final] = rd[:final]
        costs[q][:num] = L.costs(0)
        costs[q][8:8 + len(had_c)] = had_c
    return satd, lists, costs


def main():
    D = driver()
    out = {}
    for bd, s in SETS.items():
        rng = np.random.default_rng(8400 + bd)
        case = imc.make_case(rng, bd, s["specs"], s["lam"], s["flags"])
        satd, lists, costs = ref_pass(D, case, s["flags"], s["lam"])
        seen = set()
        r = imc.restate(case, s["flags"], s["lam"], seen=seen)               # the restatement reproduces every stored value
        assert np.array_equal(r["satd"], satd), bd
        assert np.array_equal(r["lists"], lists), (bd, r["lists"], lists)
        assert r["costs"].tobytes() == costs.tobytes(), bd
        assert {"MPM in the list", "even MPM appended", "unevaluated odd MPM appended", "shared child", "all 35 SATDs equal", "PBINTRA 0", "PBINTRA 1",
                "PBINTRA 2", "PBINTRA uncut"} <= seen, sorted(seen)
        k = "bd%d_" % bd
        out.update({k + "rec": case.rec, k + "org": case.org, k + "pus": case.pus.view(np.uint8), k + "avail": case.avail, k + "flags": np.int32(s["flags"]),
                    k + "sqrt_lambda": np.float64(s["lam"]), k + "refs": r["refs"], k + "satd": satd, k + "lists": lists, k + "costs": costs})
        print("bit depth %d: %d PUs, final list sizes %s, branches %s" % (bd, len(case.pus), sorted(int(v) for v in set(lists[:, 0])), sorted(seen)))
    path = os.path.join(HERE, "intra_mode_cand.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) <= 400 * 1024


if __name__ == "__main__":
    main()
