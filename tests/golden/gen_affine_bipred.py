"""Generates tests/golden/affine_bipred.npz: whole affine bi-predictive searches (the bi-predictive part of InterSearch::xPredAffineInterSearch,
InterSearch.cpp:2823-2997) whose every step is the COMPILED REFERENCE's.  Build machine only (needs the reference tree and oracle/_ref/libvtmref.so,
i.e. a build() where the reference exists):  python tests/golden/gen_affine_bipred.py

xPredAffineInterSearch itself needs the affine AMVP derivation, the uni-predictive stage and the mode control around it, which is no modest scaffold;
so gen_affine_bipred_driver.cpp -- compiled here against the reference's headers (the include set of oracle/Makefile's CXXFLAGS_REF,
-fno-access-control) and linked with libvtmref.so -- exposes the reference's own xAffineMotionEstimation(bBi = true), xCheckBestAffineMVP and the luma
motionCompensation of an affine PU after PU::setAllAffineMv on a real Picture / Slice / PU scaffold, and ref_loop() below drives them with the loop
control of :2823-2997, written here from the reference's text.  The tests' restatement (tests/affine_bipred_cases.py) has its own writing of that loop
control over the CPU restatement's pixel steps; the generator asserts that it reproduces every stored result and every trace entry.  So the arithmetic
of every step is the compiled reference's, and the loop control is pinned by two independent drivings of it.  Nothing of the reference is copied; only
the resulting data is stored.  The `steps` of the trace (which xAffineMotionEstimation does not return) are the restatement's, stored after
everything else agreed.  xCheckBestAffineMVP has no CHECK, so every generated item is stored."""
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

import affine_bipred_cases as ac  # noqa: E402
import pu_search_kit as kit  # noqa: E402
from oraclelib import p  # noqa: E402
from vvcsoftware_vtm_amd import abi  # noqa: E402

REF = os.environ.get("REF", "/root/reference")
W, H = 256, 128
N_PLANES = 4
FLAT = (192, 64, 64, 64)             # x, y, w, h of the flat patch of the original
MVP_IDX_COST = (1, 1, 0)
SHAPES = [(16, 16), (32, 32), (64, 32), (32, 64), (128, 16), (16, 128), (128, 128)]
#          num_iter, pick_list_by_cost, mvd_l1_zero, clip_key, affine_type | n_ref
GROUPS = [((4, 0, 0, 1, 1), (2, 2)),
          ((4, 0, 0, 0, 1), (4, 1)),
          ((1, 1, 0, 1, 1), (1, 2)),
          ((1, 0, 1, 1, 1), (2, 4)),
          ((4, 0, 0, 1, 0), (2, 2))]
NEED = ["mvp_switch", "closing_changes_bits", "nonzero_ref_accepted", "full_limit", "zero_delta_stop", "flat", ("passes", 2), ("passes", 3),
        ("passes", 4), ("closing", 0), ("closing", 1), ("six", 0), ("six", 1), "only_ref"] + [("shape",) + s for s in SHAPES]


def driver():
    src = os.path.join(REF, "source", "Lib")
    inc = ["-I" + os.path.join(src, d) for d in ("", "CommonLib", "CommonLib/x86", "libmd5", "EncoderLib", "DecoderLib", "Utilities")]
    refdir = os.path.join(ROOT, "oracle", "_ref")
    out = os.path.join(tempfile.mkdtemp(), "libabref.so")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-fPIC", "-shared", "-msse4.1", "-w", "-DNDEBUG", "-fno-access-control"] + inc +
                          [os.path.join(HERE, "gen_affine_bipred_driver.cpp"), "-o", out, "-L" + refdir, "-lvtmref", "-Wl,-rpath," + refdir])
    return C.CDLL(out)


def ref_loop(D, org, it, flags):
    """:2823-2997 over the driver's primitives -> (result record, trace records without `steps`, facts)"""
    num_iter, pick, mvd_l1_zero = flags[:3]
    px, py, w, h, six = int(it["pos_x"]), int(it["pos_y"]), int(it["w"]), int(it["h"]), int(it["six_param"])
    blk = org.reshape(-1)[int(it["org_off"]):]
    n_ref = [int(v) for v in it["n_ref"]]
    rec = it["ref"]
    planes0, planes1 = np.ascontiguousarray(rec[0]["plane"].astype(np.int32)), np.ascontiguousarray(rec[1]["plane"].astype(np.int32))
    D.abref_set_lists(n_ref[0], p(planes0), n_ref[1], p(planes1))
    cMvTemp = [[kit.vec3(rec[l][r]["mv"]) for r in range(4)] for l in range(2)]
    aaiMvpIdxBi = [[int(rec[l][r]["mvp_idx"]) for r in range(4)] for l in range(2)]
    cMvPredBi = [[kit.vec3(rec[l][r]["mv_cand"][aaiMvpIdxBi[l][r]]) for r in range(4)] for l in range(2)]
    cMvBi = [kit.vec3(it["mv"][l]) for l in range(2)]
    iRefIdxBi = [int(v) for v in it["ref_idx"]]
    uiCost = [int(v) for v in it["cost"]]
    uiMbBits = [int(v) for v in it["mb_bits"]]
    refIdx4Para = [int(v) for v in it["only_ref"]]

    def mc(lst):
        D.abref_mc(px, py, w, h, six, lst, iRefIdxBi[lst], p(np.array(cMvBi[lst], np.int32)), None)

    uiMotBits = [int(it["bits"][0]) - uiMbBits[0], int(it["bits"][1]) - uiMbBits[1]]
    if mvd_l1_zero:                                                             # :2840-2876 (bestBiPRefIdxL1 = ref_idx[1], bestBiPMvpL1 = its mvp_idx)
        best = iRefIdxBi[1]
        cand = kit.vec3(rec[1][best]["mv_cand"][aaiMvpIdxBi[1][best]])
        cMvPredBi[1][best], cMvBi[1], cMvTemp[1][best] = [list(v) for v in cand], [list(v) for v in cand], [list(v) for v in cand]
        mc(1)
        uiMotBits[1] = uiMbBits[1]
        if n_ref[1] > 1:
            uiMotBits[1] += best + 1
            if best == n_ref[1] - 1:
                uiMotBits[1] -= 1
        uiMotBits[1] += MVP_IDX_COST[aaiMvpIdxBi[1][best]]
    uiBits2 = uiMbBits[2] + uiMotBits[0] + uiMotBits[1]
    uiCostBi = (1 << 64) - 1
    trace, facts = np.zeros(ac.MAX_STEPS, abi.AFFINE_BIPRED_STEP), set()
    calls = closing = 0

    def check(lst, a, mv, pred, idx, bits, cost):
        pr, ix, b, c = np.array(pred, np.int32), C.c_int(idx), C.c_uint(bits & ac.U32), C.c_uint64(cost)
        cands = np.ascontiguousarray(a["mv_cand"].astype(np.int32).reshape(-1))
        D.abref_check_best_mvp(six, lst, p(np.array(mv, np.int32)), p(pr), C.byref(ix), p(cands), int(a["num_cand"]), C.byref(b), C.byref(c))
        return kit.vec3(pr), ix.value, b.value, c.value

    for iIter in range(num_iter):
        iRefList = iIter % 2
        if pick:
            iRefList = 1 if uiCost[0] <= uiCost[1] else 0
        elif iIter == 0:
            iRefList = 0
        if iIter == 0 and not mvd_l1_zero:
            mc(1 - iRefList)
        if mvd_l1_zero:
            iRefList = 0
        bChanged = False
        for iRefIdxTemp in range(n_ref[iRefList]):
            if six and refIdx4Para[iRefList] != iRefIdxTemp:
                continue
            uiBitsTemp = uiMbBits[2] + uiMotBits[1 - iRefList]
            if n_ref[iRefList] > 1:
                uiBitsTemp += iRefIdxTemp + 1
                if iRefIdxTemp == n_ref[iRefList] - 1:
                    uiBitsTemp -= 1
            uiBitsTemp += MVP_IDX_COST[aaiMvpIdxBi[iRefList][iRefIdxTemp]]
            mv, bits, cost = np.array(cMvTemp[iRefList][iRefIdxTemp], np.int32), C.c_uint(uiBitsTemp & ac.U32), C.c_uint64(0)
            mvp = np.array(cMvPredBi[iRefList][iRefIdxTemp], np.int32)
            D.abref_me(p(blk), int(it["org_stride"]), px, py, w, h, six, iRefList, iRefIdxTemp, p(mvp), p(mv), C.byref(bits), C.byref(cost))
            cMvTemp[iRefList][iRefIdxTemp] = kit.vec3(mv)
            before = aaiMvpIdxBi[iRefList][iRefIdxTemp]
            cMvPredBi[iRefList][iRefIdxTemp], aaiMvpIdxBi[iRefList][iRefIdxTemp], uiBitsTemp, uiCostTemp = check(
                iRefList, rec[iRefList][iRefIdxTemp], cMvTemp[iRefList][iRefIdxTemp], cMvPredBi[iRefList][iRefIdxTemp], before, bits.value, cost.value)
            if aaiMvpIdxBi[iRefList][iRefIdxTemp] != before:
                facts.add("mvp_switch")
            accepted = uiCostTemp < uiCostBi
            trace[calls] = (iRefList, iRefIdxTemp, cMvTemp[iRefList][iRefIdxTemp], 0, uiBitsTemp, aaiMvpIdxBi[iRefList][iRefIdxTemp], int(accepted), uiCostTemp)
            calls += 1
            if accepted:
                bChanged = True
                if iRefIdxTemp > 0:
                    facts.add("nonzero_ref_accepted")
                cMvBi[iRefList] = [list(v) for v in cMvTemp[iRefList][iRefIdxTemp]]
                iRefIdxBi[iRefList] = iRefIdxTemp
                uiCostBi = uiCostTemp
                uiMotBits[iRefList] = uiBitsTemp - uiMbBits[2] - uiMotBits[1 - iRefList]
                uiBits2 = uiBitsTemp
                if num_iter != 1:
                    mc(iRefList)
        if not bChanged:
            if uiCostBi <= uiCost[0] and uiCostBi <= uiCost[1]:
                closing, b0 = 1, uiBits2
                r0 = iRefIdxBi[0]
                cMvPredBi[0][r0], aaiMvpIdxBi[0][r0], uiBits2, uiCostBi = check(0, rec[0][r0], cMvBi[0], cMvPredBi[0][r0], aaiMvpIdxBi[0][r0], uiBits2, uiCostBi)
                if not mvd_l1_zero:
                    r1 = iRefIdxBi[1]
                    cMvPredBi[1][r1], aaiMvpIdxBi[1][r1], uiBits2, uiCostBi = check(1, rec[1][r1], cMvBi[1], cMvPredBi[1][r1], aaiMvpIdxBi[1][r1], uiBits2, uiCostBi)
                if uiBits2 != b0:
                    facts.add("closing_changes_bits")
            break
    res = np.zeros(1, abi.AFFINE_BIPRED_RESULT)
    res[0] = (cMvBi, iRefIdxBi, [aaiMvpIdxBi[l][iRefIdxBi[l]] for l in range(2)], [cMvPredBi[l][iRefIdxBi[l]] for l in range(2)], uiBits2 & ac.U32,
              [v & ac.U32 for v in uiMotBits], calls, closing, 0, uiCostBi)
    return res[0], trace, facts


def build_items(rng, searcher, org, bd, n_ref):
    """the items of one group, with tags; "near" items paint the original and carry high uni costs, so that the closing checks run where the loop stops
    early and meet a list whose vector the loop never accepted"""
    items, tags = [], []
    scales = [(0.05, 0.6), (0.5, 1.4), (2.0, 30.0)]
    for (w, h) in SHAPES:
        for six in (0, 1):
            for near in (0, 1):
                px = int(rng.integers(0, (W - 64 - w) // 4 + 1)) * 4 if w <= W - 64 else 0        # the flat patch stays as it is
                py = int(rng.integers(0, (H - h) // 4 + 1)) * 4
                it = ac.random_item(rng, W, H, bd, w, h, six, n_ref, N_PLANES, px, py, cost_scale=scales[2 if near else int(rng.integers(0, 3))],
                                    one_cand=(w, h, six, near) == (32, 32, 0, 0))
                if near:
                    ac.paint(org, searcher, it, rng)
                items.append(it)
                tags.append("near" if near else "far")
    # aacMv[1] a little off the list-1 record's entry vectors: where the list-1 pass moves but is not accepted, the closing check meets a vector the
    # loop's own checks never saw
    for k in range(8):
        w, h = [(16, 16), (32, 32)][k % 2]
        it = ac.random_item(rng, W, H, bd, w, h, (k >> 1) & 1, n_ref, N_PLANES, int(rng.integers(0, (W - 64 - w) // 4 + 1)) * 4,
                            int(rng.integers(0, (H - h) // 4 + 1)) * 4, cost_scale=scales[2])
        it["mv"][1] += rng.integers(-3, 4, (3, 2)).astype(np.int32) * 4
        ac.paint(org, searcher, it, rng)
        items.append(it)
        tags.append("quirk")
    fx, fy, _, _ = FLAT
    for six in (0, 1):
        items.append(ac.random_item(rng, W, H, bd, 16 << six, 16, six, n_ref, N_PLANES, fx + 16, fy + 16, cost_scale=(2.0, 30.0)))
        tags.append("flat")
    return np.array(items, dtype=abi.AFFINE_BIPRED_ITEM), tags


def build_set(D, bd, rng):
    mx = (1 << bd) - 1
    lam = 37.5 if bd == 10 else 11.25
    planes, org = kit.planes_and_mean_org(rng, N_PLANES, W, H, bd)
    fx, fy, fw, fh = FLAT
    org[fy:fy + fh, fx:fx + fw] = mx // 3 + 7                                        # flat original on flat references: zero gradients, a singular system
    for k in range(N_PLANES):
        planes[k, fy:fy + fh, fx:fx + fw] = mx // 3 + 7 + 3 * k
    painter = ac.Searcher(org, kit.pad(planes), ac.cfg_dict(lam, W, H, bd))
    groups = [build_items(rng, painter, org, bd, n_ref) for _, n_ref in GROUPS]      # "near" items paint the original: all items first
    org = np.ascontiguousarray(org)
    cost = np.array(MVP_IDX_COST, np.uint32)
    items, group, want, trace, tags, facts = [], [], [], [], [], set()
    for gi, ((flags, n_ref), (its, tg)) in enumerate(zip(GROUPS, groups)):
        D.abref_open(p(planes), N_PLANES, W, H, bd, C.c_double(lam), flags[3], flags[4], p(cost))
        for it, tag in zip(its, tg):
            r, t, f = ref_loop(D, org, it, flags)
            items.append(it); group.append(gi); want.append(r); trace.append(t); tags.append(tag)
            facts |= f
    return (planes, org, np.array(items, dtype=abi.AFFINE_BIPRED_ITEM), np.array(group, np.int32), lam, np.array(want, dtype=abi.AFFINE_BIPRED_RESULT),
            np.array(trace, dtype=abi.AFFINE_BIPRED_STEP), tags, facts)


def check_set(bd, planes, org, items, group, lam, want, trace, tags, facts):
    """the restatement reproduces every reference result and trace entry (and supplies `steps`); the set holds the cases the tests rely on"""
    pp = kit.pad(planes)
    for gi, (flags, n_ref) in enumerate(GROUPS):
        cfg = ac.cfg_dict(lam, W, H, bd, mvp_idx_cost=MVP_IDX_COST, **dict(zip(ac.GOLDEN_FLAGS, flags)))
        s = ac.Searcher(org, pp, cfg)
        for i in np.nonzero(group == gi)[0]:
            it = items[i]
            res, tr = s.search(it, facts)
            assert res.tobytes() == want[i].tobytes(), (bd, i, tags[i], res, want[i])
            got = tr.copy()
            got["steps"] = 0
            assert np.array_equal(got, trace[i]), (bd, i, tags[i], got, trace[i])
            trace[i] = tr
            n = int(res["me_calls"])
            facts |= {("shape", int(it["w"]), int(it["h"])), ("passes", kit.passes(tr, n)), ("closing", int(res["closing"])), ("six", int(it["six_param"]))}
            if int(it["six_param"]) and min(int(v) for v in it["only_ref"]) >= 0:
                facts.add("only_ref")
            if tags[i] == "flat":
                assert (tr["steps"][:n] == 1).all(), (bd, i)                              # every search stops on the zero deltas of its first solve
                facts.add("flat")
    for f in NEED:
        assert f in facts, (bd, f, sorted(map(str, facts)))


def main():
    D = driver()
    out = {}
    for bd in (10, 8):
        rng = np.random.default_rng(int(os.environ.get("SEED", "6101")) + bd)
        planes, org, items, group, lam, want, trace, tags, facts = build_set(D, bd, rng)
        check_set(bd, planes, org, items, group, lam, want, trace, tags, facts)
        k = "bd%d_" % bd
        out.update({k + "planes": planes, k + "org": org, k + "items": items, k + "group": group, k + "flags": np.array([g[0] for g in GROUPS], np.int32),
                    k + "lambda": np.float64(lam), k + "mvp_idx_cost": np.array(MVP_IDX_COST, np.uint32), k + "want": want, k + "trace": trace})
        ps = [kit.passes(trace[i], want[i]["me_calls"]) for i in range(len(items))]
        print("bit depth %d: %d items, passes %s, closing %d" % (bd, len(items), np.bincount(ps), int(want["closing"].sum())))
    path = os.path.join(HERE, "affine_bipred.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
