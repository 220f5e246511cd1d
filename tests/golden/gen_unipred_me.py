"""Generates tests/golden/unipred_me.npz: whole uni-predictive stages (the loop of InterSearch::predInterSearch, InterSearch.cpp:877-964) whose every
step is the COMPILED REFERENCE's.  Build machine only (needs the reference tree and oracle/_ref/libvtmref.so, i.e. a build() where the reference
exists):  python tests/golden/gen_unipred_me.py

predInterSearch itself needs the AMVP derivation, the motion buffers of a CodingStructure and the mode control around it, which is no modest scaffold;
so gen_unipred_me_driver.cpp -- compiled here against the reference's headers (the include set of oracle/Makefile's CXXFLAGS_REF,
-fno-access-control) and linked with libvtmref.so -- exposes the reference's own xEstimateMvPredAMVP(bFilled = true), xMotionEstimation(bBi = false),
xCheckBestMVP and the two RdCost calls of the list-1 shortcut on a real Picture / Slice / PU scaffold, and ref_loop() below drives them with the loop
control of :877-964 (and :1009-1023, :1038 for the out-item), written here from the reference's text.  The tests' restatement
(tests/unipred_me_cases.py) has its own writing of that loop control over the CPU restatement's pixel steps; the generator asserts that it reproduces
every stored result and out-item.  Nothing of the reference is copied; only the resulting data is stored.

The cached-start path (:1759-1766) needs a CacheBlkInfoCtrl, i.e. an EncModeCtrl with its coding-structure stack, which this scaffold does not hold:
the golden set does not cover it.  The restatement alone pins that path (tests/test_unipred_me_cpu.py), on top of the fast-settings searches that
tests/golden/tzsearch.npz pins to the reference.

Items on which the reference throws are outside the entry's contract: they are dropped and counted, and may be at most a quarter."""
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

import unipred_me_cases as uc  # noqa: E402
import pu_search_kit as kit  # noqa: E402
from oraclelib import p  # noqa: E402
from vvcsoftware_vtm_amd import abi  # noqa: E402

REF = os.environ.get("REF", "/root/reference")
W, H = 256, 128
N_PLANES = 4
FLAT = (192, 64, 64, 64)             # x, y, w, h of the flat patch of the original
MVP_IDX_COST = (1, 1, 0)
U64 = (1 << 64) - 1
# slice-level settings of a group; fast: sub_shift 1 where h > 8 and w <= 64; ext: MESEARCH_DIAMOND_ENHANCED; shapes: how many of the 36 side pairs
GROUPS = [dict(n_ref=(2, 2), ref_plane=((0, 1, 0, 0), (1, 2, 0, 0)), search_range=((32, 32, 1, 1), (32, 8, 1, 1)), list1_to_list0=(0, -1, -1, -1), fast_me=1, mvd=0,
               fss=0, had=1, fast=0, ext=0, shapes=36),
          dict(n_ref=(4, 1), ref_plane=((0, 1, 2, 3), (2, 0, 0, 0)), search_range=((8, 8, 8, 8), (8, 1, 1, 1)), list1_to_list0=(-1, -1, -1, -1), fast_me=0, mvd=0,
               fss=1, had=0, fast=1, ext=1, shapes=18),
          dict(n_ref=(1, 2), ref_plane=((3, 0, 0, 0), (0, 1, 0, 0)), search_range=((32, 1, 1, 1), (8, 32, 1, 1)), list1_to_list0=(-1, -1, -1, -1), fast_me=1, mvd=1,
               fss=0, had=1, fast=1, ext=0, shapes=18),
          dict(n_ref=(2, 0), ref_plane=((1, 3, 0, 0), (0, 0, 0, 0)), search_range=((8, 32, 1, 1), (1, 1, 1, 1)), list1_to_list0=(-1, -1, -1, -1), fast_me=0, mvd=0,
               fss=0, had=1, fast=0, ext=1, shapes=18),
          dict(n_ref=(2, 4), ref_plane=((0, 2, 0, 0), (1, 0, 3, 2)), search_range=((32, 32, 1, 1), (32, 32, 8, 8)), list1_to_list0=(-1, 0, 1, -1), fast_me=1, mvd=1,
               fss=0, had=0, fast=0, ext=0, shapes=18)]


def group_cfg(g, lam, bd):
    return uc.cfg_dict(lam, W, H, bd, n_ref=g["n_ref"], ref_plane=g["ref_plane"], search_range=g["search_range"], list1_to_list0=g["list1_to_list0"],
                       fast_me_gen_b_low_delay=g["fast_me"], mvd_l1_zero=g["mvd"], first_search_stop=g["fss"], use_hadamard=g["had"], mvp_idx_cost=MVP_IDX_COST)


def driver():
    src = os.path.join(REF, "source", "Lib")
    inc = ["-I" + os.path.join(src, d) for d in ("", "CommonLib", "CommonLib/x86", "libmd5", "EncoderLib", "DecoderLib", "Utilities")]
    refdir = os.path.join(ROOT, "oracle", "_ref")
    out = os.path.join(tempfile.mkdtemp(), "libupref.so")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-fPIC", "-shared", "-msse4.1", "-w", "-DNDEBUG", "-fno-access-control"] + inc +
                          [os.path.join(HERE, "gen_unipred_me_driver.cpp"), "-o", out, "-L" + refdir, "-lvtmref", "-Wl,-rpath," + refdir])
    D = C.CDLL(out)
    D.upref_vector_bits.restype = C.c_uint
    D.upref_get_cost.restype = C.c_uint64
    return D


class RefThrows(Exception):
    pass


def ref_loop(D, org, it, grp):
    """:877-964 over the driver's primitives -> (result record, out-item record); raises RefThrows"""
    px, py, w, h = int(it["pos_x"]), int(it["pos_y"]), int(it["w"]), int(it["h"])
    blk, stride = org.reshape(-1)[int(it["org_off"]):], int(it["org_stride"])
    numRefIdx = grp["n_ref"]
    uiMbBits = [int(v) for v in it["mb_bits"]]
    uiCost, uiBits, iRefIdx, cMv = [U64, U64], [0, 0], [0, 0], [[0, 0], [0, 0]]
    uiCostTempL0, uiBitsTempL0 = [0] * 4, [0] * 4
    cMvTemp = [[[0, 0] for _ in range(4)] for _ in range(2)]
    aaiMvpIdx = [[0] * 4 for _ in range(2)]
    bestBiPDist, bestBiPMvpL1, bestBiPRefIdxL1 = U64, 0, 0
    costValidList1, bitsValidList1, mvValidList1, refIdxValidList1 = U64, 0xFFFFFFFF, [0, 0], 0
    res, out = np.zeros(1, abi.UNIPRED_ME_RESULT), np.zeros(1, abi.BIPRED_ME_ITEM)
    for iRefList in range(2):
        for iRefIdxTemp in range(numRefIdx[iRefList]):
            a = it["ref"][iRefList][iRefIdxTemp]
            cands = np.ascontiguousarray(a["mv_cand"].astype(np.int32).reshape(-1))
            numCand = int(a["num_cand"])
            uiBitsTemp = uiMbBits[iRefList]
            if numRefIdx[iRefList] > 1:
                uiBitsTemp += iRefIdxTemp + 1
                if iRefIdxTemp == numRefIdx[iRefList] - 1:
                    uiBitsTemp -= 1
            cMvPred, mvpIdx, biPDistTemp, tmpl = np.zeros(2, np.int32), C.c_int(0), C.c_uint64(0), np.zeros(2, np.uint64)
            if D.upref_amvp(p(blk), stride, px, py, w, h, iRefList, iRefIdxTemp, p(cands), numCand, p(cMvPred), C.byref(mvpIdx), C.byref(biPDistTemp), p(tmpl)):
                raise RefThrows()
            aaiMvpIdx[iRefList][iRefIdxTemp] = mvpIdx.value
            if grp["mvd"] and iRefList == 1 and biPDistTemp.value < bestBiPDist:
                bestBiPDist, bestBiPMvpL1, bestBiPRefIdxL1 = biPDistTemp.value, aaiMvpIdx[iRefList][iRefIdxTemp], iRefIdxTemp
            uiBitsTemp += MVP_IDX_COST[aaiMvpIdx[iRefList][iRefIdxTemp]]
            intMv = np.zeros(2, np.int32)
            if grp["fast_me"] and iRefList == 1 and grp["list1_to_list0"][iRefIdxTemp] >= 0:
                k = grp["list1_to_list0"][iRefIdxTemp]
                cMvTemp[1][iRefIdxTemp] = list(cMvTemp[0][k])
                uiCostTemp = uiCostTempL0[k]
                uiCostTemp = (uiCostTemp - D.upref_get_cost(uiBitsTempL0[k])) & U64
                uiBitsTemp += D.upref_vector_bits(p(cMvPred), p(np.array(cMvTemp[1][iRefIdxTemp], np.int32)))
                uiCostTemp = (uiCostTemp + D.upref_get_cost(uiBitsTemp)) & U64
            else:
                mv, bits, cost = np.zeros(2, np.int32), C.c_uint(uiBitsTemp), C.c_uint64(0)
                pred2 = np.ascontiguousarray(a["pred2"].astype(np.int32)) if int(a["flags"]) & abi.UNIPRED_PRED2 else None
                if D.upref_me(p(blk), stride, px, py, w, h, iRefList, iRefIdxTemp, p(cMvPred), p(pred2), p(mv), p(intMv), aaiMvpIdx[iRefList][iRefIdxTemp],
                              C.byref(bits), C.byref(cost)):
                    raise RefThrows()
                cMvTemp[iRefList][iRefIdxTemp], uiBitsTemp, uiCostTemp = [int(mv[0]), int(mv[1])], bits.value, cost.value
            pr, ix, b, c = cMvPred.copy(), C.c_int(aaiMvpIdx[iRefList][iRefIdxTemp]), C.c_uint(uiBitsTemp), C.c_uint64(uiCostTemp)
            if D.upref_check_best_mvp(iRefList, p(np.array(cMvTemp[iRefList][iRefIdxTemp], np.int32)), p(pr), C.byref(ix), p(cands), numCand, C.byref(b), C.byref(c)):
                raise RefThrows()
            aaiMvpIdx[iRefList][iRefIdxTemp], uiBitsTemp, uiCostTemp = ix.value, b.value, c.value
            res[0]["s"][iRefList][iRefIdxTemp] = (cMvTemp[iRefList][iRefIdxTemp], intMv, ix.value, uiBitsTemp, uiCostTemp, tmpl)
            if iRefList == 0:
                uiCostTempL0[iRefIdxTemp], uiBitsTempL0[iRefIdxTemp] = uiCostTemp, uiBitsTemp
            if uiCostTemp < uiCost[iRefList]:
                uiCost[iRefList], uiBits[iRefList] = uiCostTemp, uiBitsTemp
                cMv[iRefList], iRefIdx[iRefList] = list(cMvTemp[iRefList][iRefIdxTemp]), iRefIdxTemp
            if iRefList == 1 and uiCostTemp < costValidList1 and grp["list1_to_list0"][iRefIdxTemp] < 0:
                costValidList1, bitsValidList1 = uiCostTemp, uiBitsTemp
                mvValidList1, refIdxValidList1 = list(cMvTemp[iRefList][iRefIdxTemp]), iRefIdxTemp
    r = res[0]
    r["ref_idx"], r["mv"], r["cost"], r["bits"] = iRefIdx, cMv, uiCost, uiBits
    r["best_bip_ref_idx_l1"], r["best_bip_mvp_l1"], r["best_bip_dist"] = bestBiPRefIdxL1, bestBiPMvpL1, bestBiPDist
    r["valid_l1_ref_idx"], r["valid_l1_mv"], r["valid_l1_bits"], r["valid_l1_cost"] = refIdxValidList1, mvValidList1, bitsValidList1, costValidList1
    # the items of the bi-predictive entry: what :1000-1038 set up from the above
    o = out[0]
    for f in ("pos_x", "pos_y", "w", "h", "sub_shift", "org_off", "org_stride", "mb_bits"):
        o[f] = it[f]
    o["n_ref"], o["ref_idx"], o["mv"], o["cost"], o["bits"] = numRefIdx, iRefIdx, cMv, uiCost, uiBits
    for l in range(2):
        for k in range(numRefIdx[l]):
            q = o["ref"][l][k]
            q["plane"], q["mv"], q["mv_cand"], q["num_cand"], q["mvp_idx"] = grp["ref_plane"][l][k], cMvTemp[l][k], it["ref"][l][k]["mv_cand"], it["ref"][l][k]["num_cand"], aaiMvpIdx[l][k]
    if grp["mvd"] and numRefIdx[1] > 0:
        q = o["ref"][1][bestBiPRefIdxL1]
        q["mvp_idx"] = bestBiPMvpL1                                # aaiMvpIdxBi[1][bestBiPRefIdxL1] = bestBiPMvpL1
        q["mv"] = q["mv_cand"][bestBiPMvpL1]                       # cMvTemp[1][bestBiPRefIdxL1] = cMvBi[1] = the candidate
        o["mv"][1], o["ref_idx"][1] = q["mv"], bestBiPRefIdxL1
    return res[0], out[0]


def build_items(rng, grp, gi):
    """the candidate items of one group"""
    items = []
    n_ref = grp["n_ref"]

    def recs(base, far=0, shared=False):
        out = []
        one = [list(base + rng.integers(-9, 10, 2)) for _ in range(int(rng.integers(1, 3)))]
        for l in range(2):
            rr = []
            for r in range(4):
                b = base + far * rng.choice([-1, 1], 2)
                cands = one if shared else [list(b + rng.integers(-9, 10, 2)) for _ in range(int(rng.integers(1, 3)))]
                rr.append((cands, int(rng.choice([0, abi.UNIPRED_PRED2])), list(rng.integers(-12, 13, 2)), [0, 0]))
            out.append(rr)
        return out

    def add(px, py, w, h, refs):
        items.append(uc.item(px, py, w, h, kit.sub_shift_of(w, h, grp["fast"]), py * W + px, W, refs, abi.TZ_EXTENDED * grp["ext"], [int(v) for v in rng.integers(1, 6, 3)]))

    shapes = uc.all_shapes()
    pick = shapes if grp["shapes"] >= len(shapes) else [shapes[(5 * gi + 2 * k) % len(shapes)] for k in range(grp["shapes"])]
    for (w, h) in pick:
        px = int(rng.integers(0, (W - 64 - w) // 4 + 1)) * 4 if w <= W - 64 else 0
        py = int(rng.integers(0, (H - h) // 4 + 1)) * 4
        add(px, py, w, h, recs(np.array([20, -12]) + rng.integers(-16, 17, 2)))
    # picture corners, candidates far outside: clipMv binds
    for (px, py, w, h) in [(0, 0, 32, 32), (W - 16, H - 16, 16, 16), (0, H - 8, 8, 8), (W - 64, 0, 64, 16)]:
        add(px, py, w, h, recs(np.zeros(2, np.int64), far=int(rng.integers(2500, 5000))))
    # flat original
    fx, fy, _, _ = FLAT
    add(fx + 16, fy + 16, 16, 16, recs(rng.integers(-8, 9, 2)))
    add(fx + 32, fy + 8, 8, 32, recs(rng.integers(-8, 9, 2), shared=True))
    return np.array(items, dtype=abi.UNIPRED_ME_ITEM)


def build_set(D, bd, rng):
    mx = (1 << bd) - 1
    lam = 37.5 if bd == 10 else 11.25
    planes = np.stack([kit.texture(rng, H, W, bd, 1.5 * k) for k in range(N_PLANES)])
    org = np.clip(np.roll(planes[0], (3, -5), axis=(0, 1)).astype(np.int32) + rng.integers(-5, 6, (H, W)), 0, mx).astype(np.int16)
    fx, fy, fw, fh = FLAT
    org[fy:fy + fh, fx:fx + fw] = mx // 3 + 7
    org = np.ascontiguousarray(org)
    cost = np.array(MVP_IDX_COST, np.uint32)
    items, group, want, outs = [], [], [], []
    generated = dropped = 0
    for gi, grp in enumerate(GROUPS):
        D.upref_open(p(planes), N_PLANES, W, H, bd, C.c_double(lam), grp["had"], grp["fast"], grp["ext"], grp["fss"], p(cost))
        a = [np.array(grp[k][l], np.int32) for k in ("ref_plane", "search_range") for l in range(2)]
        D.upref_set_lists(grp["n_ref"][0], p(a[0]), p(a[2]), grp["n_ref"][1], p(a[1]), p(a[3]))
        for it in build_items(rng, grp, gi):
            generated += 1
            try:
                r, o = ref_loop(D, org, it, grp)
            except RefThrows:
                dropped += 1
                continue
            items.append(it); group.append(gi); want.append(r); outs.append(o)
    assert dropped * 4 <= generated, (dropped, generated)
    return (planes, org, np.array(items, dtype=abi.UNIPRED_ME_ITEM), np.array(group, np.int32), lam, np.array(want, dtype=abi.UNIPRED_ME_RESULT),
            np.array(outs, dtype=abi.BIPRED_ME_ITEM), generated, dropped)


def check_set(bd, planes, org, items, group, lam, want, outs):
    """the restatement reproduces every reference result and out-item; the set holds the cases the tests rely on"""
    pp = kit.pad(planes)
    seen = set()
    for gi, grp in enumerate(GROUPS):
        cfg = group_cfg(grp, lam, bd)
        s = uc.Searcher(org, pp, cfg)
        for i in np.nonzero(group == gi)[0]:
            f = set()
            res, out = s.search(items[i], f)
            assert res.tobytes() == want[i].tobytes(), (bd, gi, i, res, want[i])
            assert out.tobytes() == outs[i].tobytes(), (bd, gi, i, out, outs[i])
            seen |= f | uc.golden_facts(org, cfg, items[i], f)
    assert uc.GOLDEN_NEED <= seen, (bd, uc.GOLDEN_NEED - seen)


def main():
    D = driver()
    out = {}
    for bd in (10, 8):
        rng = np.random.default_rng(6100 + bd)
        planes, org, items, group, lam, want, outs, generated, dropped = build_set(D, bd, rng)
        check_set(bd, planes, org, items, group, lam, want, outs)
        k = "bd%d_" % bd
        out.update({k + "planes": planes, k + "org": org, k + "items": items, k + "group": group, k + "lambda": np.float64(lam),
                    k + "mvp_idx_cost": np.array(MVP_IDX_COST, np.uint32), k + "want": want, k + "out": outs, k + "dropped": np.int32(dropped),
                    k + "generated": np.int32(generated),
                    k + "g_n_ref": np.array([g["n_ref"] for g in GROUPS], np.int32), k + "g_ref_plane": np.array([g["ref_plane"] for g in GROUPS], np.int32),
                    k + "g_search_range": np.array([g["search_range"] for g in GROUPS], np.int32),
                    k + "g_list1_to_list0": np.array([g["list1_to_list0"] for g in GROUPS], np.int32),
                    k + "g_flags": np.array([[g["fast_me"], g["mvd"], g["fss"], g["had"]] for g in GROUPS], np.int32)})
        print("bit depth %d: %d items kept of %d (the reference throws on %d)" % (bd, len(items), generated, dropped))
    path = os.path.join(HERE, "unipred_me.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
