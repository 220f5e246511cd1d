"""Generates tests/golden/merge_cand.npz: first passes of the merge analysis (EncCu::xCheckRDCostMerge2Nx2N, EncCu.cpp:1537-1612) whose every step is
the COMPILED REFERENCE's.  Build machine only (needs the reference tree and oracle/_ref/libvtmref.so, i.e. a build() where the reference exists):
    python tests/golden/gen_merge_cand.py

xCheckRDCostMerge2Nx2N itself needs the merge candidate derivation, a CodingStructure pair with its buffers and the mode control around it; so
gen_merge_cand_driver.cpp -- compiled here against the reference's headers (the include set of oracle/Makefile's CXXFLAGS_REF, -fno-access-control) and
linked with libvtmref.so -- exposes the reference's own InterPrediction::motionCompensation(pu, predBuf) for REF_PIC_LIST_X, RdCost::setDistParam(..,
bUseHadamard) + distFunc, RdCost::getDistPart(DF_SSE), the cost expression of :1599 and updateCandList, and ref_pass() below drives them with the loop
of :1568-1612, written here from the reference's text.  The tests' restatement (tests/merge_cand_cases.py) has its own writing of that loop over the CPU
restatement's pixel steps; the generator asserts that it reproduces every stored value.  Nothing of the reference is copied; only the data is stored.

Which variants were reached: CHROMA -- the scaffold is 4:2:0 (Picture::create(CHROMA_420), m_maxCompIDToPred = COMPONENT_Cr), so the chroma
predictions and their SSE are the reference's too.  ATMVP -- the calloc'ed CodingStructure is given an area and a motion buffer by hand, so an ATMVP
candidate runs the reference's own xSubPuMC (its joining of neighbours of equal motion included) over a motion field at the 4x4 granularity.

Cases have four to seven candidates: the reference's cut (:1605-1612) indexes its cost list beyond its size below four."""
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

import merge_cand_cases as mcc  # noqa: E402
from oraclelib import p  # noqa: E402

REF = os.environ.get("REF", "/root/reference")
W, H = mcc.W, mcc.H
# per bit depth: max_num_merge_cand, use_hadamard, sqrt_lambda, [(w, h, candidates, ATMVP sub-block size or 0, corner -- 5: the flat patch, 6: candidates
# around the true motion, whose costs lie close together)]
SETS = {10: dict(max_num=6, had=1, lam=27.375,
                 shapes=[(8, 8, 5, 0, 0), (4, 8, 4, 0, 0), (16, 16, 7, 4, 0), (32, 32, 6, 8, 0), (64, 64, 4, 0, 0), (128, 16, 4, 0, 0), (16, 4, 5, 0, 0),
                         (8, 32, 6, 4, 0), (32, 8, 7, 0, 6), (16, 16, 5, 0, 1), (32, 16, 4, 0, 2), (16, 16, 6, 0, 5), (16, 8, 5, 0, 6), (8, 8, 6, 0, 6)]),
        8: dict(max_num=7, had=1, lam=8.5,
                shapes=[(4, 4, 7, 0, 0), (8, 16, 5, 4, 0), (16, 8, 6, 8, 0), (64, 32, 5, 8, 0), (16, 64, 4, 0, 0), (32, 64, 4, 0, 0), (4, 16, 6, 0, 0),
                        (64, 8, 5, 0, 6), (8, 8, 4, 8, 0), (16, 32, 7, 0, 3), (8, 8, 5, 0, 4), (16, 16, 6, 0, 5), (8, 16, 6, 0, 6), (16, 16, 4, 0, 6)])}


def driver():
    src = os.path.join(REF, "source", "Lib")
    inc = ["-I" + os.path.join(src, d) for d in ("", "CommonLib", "CommonLib/x86", "libmd5", "EncoderLib", "DecoderLib", "Utilities")]
    refdir = os.path.join(ROOT, "oracle", "_ref")
    out = os.path.join(tempfile.mkdtemp(), "libmgref.so")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-fPIC", "-shared", "-msse4.1", "-w", "-DNDEBUG", "-fno-access-control"] + inc +
                          [os.path.join(HERE, "gen_merge_cand_driver.cpp"), "-o", out, "-L" + refdir, "-lvtmref", "-Wl,-rpath," + refdir])
    D = C.CDLL(out)
    D.mgref_dist.restype = D.mgref_sse.restype = C.c_uint64
    D.mgref_cost.restype = C.c_double
    return D


def motion_ints(cand, w, h):
    """the driver's motion argument of a candidate: eight ints, or eight per 4x4 unit of the PU for an ATMVP candidate"""
    if cand[0] == "default":
        return np.array(mcc._ref_ints(cand[1]) + mcc._ref_ints(cand[2]), np.int32)
    _, sub, field, _ = cand
    sw, sh = min(sub, w), min(sub, h)
    out = np.zeros((h // 4, w // 4, 8), np.int32)
    for j in range(h // 4):
        for i in range(w // 4):
            l0, l1 = field[(4 * j) // sh][(4 * i) // sw]
            out[j, i] = mcc._ref_ints(l0) + mcc._ref_ints(l1)
    return np.ascontiguousarray(out)


def ref_pass(D, fr, pus, s):
    """:1568-1612 over the driver's primitives -> (pred of every block in the order of gather_blocks, dist, sse, cost, rd_list)"""
    preds, dist, sse, cost, rows = [], [], [], [], []
    at = lambda a, off: C.c_void_p(a.ctypes.data + 2 * int(off))
    for (px, py, w, h, cands) in pus:
        modes, costs, size = np.zeros(7, np.uint32), np.zeros(7, np.float64), C.c_int(0)
        num = mcc.NUM_MRG_SATD_CAND                                       # :1527
        for k, cand in enumerate(cands):
            out = [np.zeros((h, w), np.int16), np.zeros((h // 2, w // 2), np.int16), np.zeros((h // 2, w // 2), np.int16)]
            m = motion_ints(cand, w, h)
            atmvp = cand[0] == "atmvp"
            sub_log2 = int(np.log2(cand[1])) if atmvp else 2
            assert D.mgref_mc(px, py, w, h, int(atmvp), sub_log2, p(m), int(cand[3] == 4), p(out[0]), p(out[1]), p(out[2])) == 0
            org = [at(fr.org, fr.org_off[c] + (py >> (c > 0)) * fr.org_stride[c] + (px >> (c > 0))) for c in range(3)]
            sad = D.mgref_dist(org[0], fr.org_stride[0], p(out[0]), w, w, h, 0, s["had"])
            c_ = D.mgref_cost(C.c_uint64(sad), k, s["max_num"], C.c_double(s["lam"]))
            assert D.mgref_update_cand_list(k, C.c_double(c_), p(modes), p(costs), C.byref(size), num) >= 0
            assert min(k + 1, num) == size.value                          # the CHECK of :1602
            preds += [o.reshape(-1) for o in out]
            dist.append(sad)
            cost.append(c_)
            sse.append([D.mgref_sse(org[c], fr.org_stride[c], p(out[c]), w >> (c > 0), w >> (c > 0), h >> (c > 0), c) for c in range(3)])
        for i in range(1, num):
            if costs[i] > mcc.MRG_FAST_RATIO * costs[0]:
                num = i
                break
        rows.append([num] + [int(v) for v in modes[:size.value]] + [-1] * (7 - size.value))
    return (np.concatenate(preds), np.array(dist, np.uint64), np.array(sse, np.uint64), np.array(cost, np.float64), np.array(rows, np.int32))


CORNERS = {1: (0, 0), 2: (W, 0), 3: (0, H), 4: (W, H)}


def near_cand(rng):
    """a candidate around the motion the original was made with (fresh_planes: picture 0 shifted by (-3, 2) samples; picture 2 is picture 0 shifted by
    (-7, 5)): list 0, list 1 or both, in 1/16 units with a perturbation of up to 2/16"""
    a = (0, 48 + int(rng.integers(-2, 3)), -32 + int(rng.integers(-2, 3)))
    b = (2, -64 + int(rng.integers(-2, 3)), 48 + int(rng.integers(-2, 3)))
    kind = int(rng.integers(0, 3))
    return mcc.default_cand(a if kind != 1 else None, b if kind != 0 else None, 4)


def build_pus(rng, shapes):
    pus = []
    for (w, h, n, sub, corner) in shapes:
        if corner == 5:
            px, py = mcc.FLAT[0] + 16, mcc.FLAT[1] + 16
        elif corner in (1, 2, 3, 4):
            cx, cy = CORNERS[corner]
            px, py = (cx - w if cx else 0), (cy - h if cy else 0)
        else:
            px, py = mcc.place(rng, w, h)
        if corner == 6:
            cands = [near_cand(rng) for _ in range(n)]
        else:
            cands = [mcc.random_cand(rng, w, h, far=int(rng.integers(300, 600)) if corner in (1, 2, 3, 4) else 0) for _ in range(n)]
        if sub:
            cands[int(rng.integers(0, n))] = mcc.random_cand(rng, w, h, atmvp=sub)
        if corner == 5:                                                    # equal candidates on the flat patch: equal distortions
            cands[2], cands[4] = cands[0], cands[1]
        pus.append((px, py, w, h, cands))
    return pus


def main():
    D = driver()
    out = {}
    for bd, s in SETS.items():
        rng = np.random.default_rng(7300 + bd)
        l0, l1, org = mcc.fresh_planes(rng, bd)
        fr = mcc.derived_frame(l0, l1, org, bd)
        pus = build_pus(rng, s["shapes"])
        D.mgref_open(p(np.ascontiguousarray(fr.luma)), p(np.ascontiguousarray(fr.chroma)), mcc.N_PICS, W, H, bd)
        pred, dist, sse, cost, rows = ref_pass(D, fr, pus, s)
        # the restatement reproduces every stored value
        L = mcc.layout(fr, pus)
        r = mcc.restate(fr, L, s["max_num"], s["had"], s["lam"])
        assert np.array_equal(mcc.gather_blocks(r["pred"], L), pred), bd
        assert np.array_equal(r["dist"], dist) and np.array_equal(r["sse"], sse), bd
        assert r["cost"].tobytes() == cost.tobytes() and np.array_equal(r["rd_list"], rows), (bd, r["rd_list"], rows)
        assert set(rows[:, 0]) == {1, 2, 3, 4}, rows[:, 0]     # the cut is taken at several places, and not at all
        pu, cand, field = mcc.pus_to_arrays(pus)
        again = mcc.layout(fr, mcc.pus_from_arrays(pu, cand, field))
        assert again["mc"].tobytes() == L["mc"].tobytes() and again["cand_dist"].tobytes() == L["cand_dist"].tobytes()
        k = "bd%d_" % bd
        out.update({k + "l0": l0, k + "l1": l1, k + "org": org, k + "pu": pu, k + "cand": cand, k + "field": field, k + "max_num": np.int32(s["max_num"]),
                    k + "had": np.int32(s["had"]), k + "sqrt_lambda": np.float64(s["lam"]), k + "pred": pred, k + "dist": dist, k + "sse": sse,
                    k + "cost": cost, k + "rd_list": rows})
        print("bit depth %d: %d PUs, %d candidates, %d samples, uiNumMrgSATDCand %s" % (bd, len(pus), len(dist), pred.size, sorted(int(v) for v in set(rows[:, 0]))))
    path = os.path.join(HERE, "merge_cand.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) <= os.path.getsize(os.path.join(HERE, "unipred_me.npz"))


if __name__ == "__main__":
    main()
