"""Generates tests/golden/bipred_me.npz: whole bi-predictive refinements (the loop of InterSearch::predInterSearch, InterSearch.cpp:1058-1164) whose
every step is the COMPILED REFERENCE's.  Build machine only (needs the reference tree and oracle/_ref/libvtmref.so, i.e. a build() where the reference
exists):  python tests/golden/gen_bipred_me.py

predInterSearch itself needs the AMVP derivation, the motion buffers of a CodingStructure and the mode control around it, which is no modest scaffold;
so gen_bipred_me_driver.cpp -- compiled here against the reference's headers (the include set of oracle/Makefile's CXXFLAGS_REF, -fno-access-control)
and linked with libvtmref.so -- exposes the reference's own xMotionEstimation(bBi = true), xCheckBestMVP and luma motionCompensation on a real
Picture / Slice / PU scaffold, and ref_loop() below drives them with the loop control of :1058-1164, written here from the reference's text.  The
tests' restatement (tests/bipred_me_cases.py) has its own writing of that loop control over the CPU restatement's pixel steps; the generator asserts
that it reproduces every stored result and every trace entry.  So the arithmetic of every step is the compiled reference's, and the loop control is
pinned by two independent drivings of it.  Nothing of the reference is copied; only the resulting data is stored.  The integer vectors of the trace
(which xMotionEstimation does not return) are the restatement's, stored after everything else agreed.

Items on which the reference throws (the CHECK of xCheckBestMVP, which the closing calls of :1148 / :1156 can trip because they are handed the
candidate set of the current iteration's list) are outside the entry's contract: they are dropped and counted, and may be at most a quarter."""
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

import bipred_me_cases as bc  # noqa: E402
import pu_search_kit as kit  # noqa: E402
from oraclelib import p  # noqa: E402
from vvcsoftware_vtm_amd import abi  # noqa: E402

REF = os.environ.get("REF", "/root/reference")
W, H = 256, 128
N_PLANES = 4
FLAT = (192, 64, 64, 64)             # x, y, w, h of the flat patch of the original
MVP_IDX_COST = (1, 1, 0)
NEEDED_SHAPES = [(4, 4), (4, 8), (8, 4), (16, 8), (128, 128), (128, 16), (16, 128)]
#          num_iter, pick_list_by_cost, mvd_l1_zero, search_range, clip_key, use_hadamard | fast (sub_shift 1 where h > 8 and w <= 64), n_ref
GROUPS = [((4, 0, 0, 4, 1, 1), 0, (2, 2)),
          ((4, 0, 0, 2, 0, 0), 1, (4, 1)),
          ((1, 1, 0, 4, 1, 1), 0, (1, 2)),
          ((1, 0, 1, 4, 1, 0), 1, (2, 4)),
          ((4, 0, 0, 4, 1, 1), 1, (1, 4))]


def driver():
    src = os.path.join(REF, "source", "Lib")
    inc = ["-I" + os.path.join(src, d) for d in ("", "CommonLib", "CommonLib/x86", "libmd5", "EncoderLib", "DecoderLib", "Utilities")]
    refdir = os.path.join(ROOT, "oracle", "_ref")
    out = os.path.join(tempfile.mkdtemp(), "libbpref.so")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-fPIC", "-shared", "-msse4.1", "-w", "-DNDEBUG", "-fno-access-control"] + inc +
                          [os.path.join(HERE, "gen_bipred_me_driver.cpp"), "-o", out, "-L" + refdir, "-lvtmref", "-Wl,-rpath," + refdir])
    return C.CDLL(out)


def ref_loop(D, org, it, flags):
    """:1058-1164 over the driver's primitives -> (result record, trace records without the integer vectors, facts); raises bc.RefThrows"""
    num_iter, pick, mvd_l1_zero = flags[:3]
    px, py, w, h = int(it["pos_x"]), int(it["pos_y"]), int(it["w"]), int(it["h"])
    blk = org.reshape(-1)[int(it["org_off"]):]
    n_ref = [int(v) for v in it["n_ref"]]
    rec = it["ref"]
    planes0, planes1 = np.ascontiguousarray(rec[0]["plane"].astype(np.int32)), np.ascontiguousarray(rec[1]["plane"].astype(np.int32))
    D.bpref_set_lists(n_ref[0], p(planes0), n_ref[1], p(planes1))
    cMvTemp = [[[int(v) for v in rec[l][r]["mv"]] for r in range(4)] for l in range(2)]
    aaiMvpIdxBi = [[int(rec[l][r]["mvp_idx"]) for r in range(4)] for l in range(2)]
    cMvPredBi = [[[int(v) for v in rec[l][r]["mv_cand"][aaiMvpIdxBi[l][r]]] for r in range(4)] for l in range(2)]
    cMvBi = [[int(v) for v in it["mv"][l]] for l in range(2)]
    iRefIdxBi = [int(v) for v in it["ref_idx"]]
    uiCost = [int(v) for v in it["cost"]]
    uiMbBits = [int(v) for v in it["mb_bits"]]
    uiMotBits = [int(it["bits"][0]) - uiMbBits[0], int(it["bits"][1]) - uiMbBits[1]]
    if mvd_l1_zero:                                                             # :1024-1036 (the caller has done :1009-1023)
        uiMotBits[1] = uiMbBits[1]
        if n_ref[1] > 1:
            uiMotBits[1] += iRefIdxBi[1] + 1
            if iRefIdxBi[1] == n_ref[1] - 1:
                uiMotBits[1] -= 1
        uiMotBits[1] += MVP_IDX_COST[aaiMvpIdxBi[1][iRefIdxBi[1]]]
        D.bpref_mc(px, py, w, h, 1, iRefIdxBi[1], cMvBi[1][0], cMvBi[1][1], None)   # :1021-1022
    uiBits2 = uiMbBits[2] + uiMotBits[0] + uiMotBits[1]
    uiCostBi = (1 << 64) - 1
    trace, facts = np.zeros(bc.MAX_STEPS, abi.BIPRED_ME_STEP), set()
    calls = closing = 0

    def check(lst, a, mv, pred, idx, bits, cost):
        pr, ix, b, c = np.array(pred, np.int32), C.c_int(idx), C.c_uint(bits), C.c_uint64(cost)
        cands = np.ascontiguousarray(a["mv_cand"].astype(np.int32).reshape(-1))
        mva = np.array(mv, np.int32)
        if D.bpref_check_best_mvp(lst, p(mva), p(pr), C.byref(ix), p(cands), int(a["num_cand"]), C.byref(b), C.byref(c)):
            raise bc.RefThrows()
        return [int(pr[0]), int(pr[1])], ix.value, b.value, c.value

    for iIter in range(num_iter):
        iRefList = iIter % 2
        if pick:
            iRefList = 1 if uiCost[0] <= uiCost[1] else 0
        elif iIter == 0:
            iRefList = 0
        if iIter == 0 and not mvd_l1_zero:
            o = 1 - iRefList
            D.bpref_mc(px, py, w, h, o, iRefIdxBi[o], cMvBi[o][0], cMvBi[o][1], None)
        if mvd_l1_zero:
            iRefList = 0
        bChanged = False
        for iRefIdxTemp in range(n_ref[iRefList]):
            uiBitsTemp = uiMbBits[2] + uiMotBits[1 - iRefList]
            if n_ref[iRefList] > 1:
                uiBitsTemp += iRefIdxTemp + 1
                if iRefIdxTemp == n_ref[iRefList] - 1:
                    uiBitsTemp -= 1
            uiBitsTemp += MVP_IDX_COST[aaiMvpIdxBi[iRefList][iRefIdxTemp]]
            mv, bits, cost = np.array(cMvTemp[iRefList][iRefIdxTemp], np.int32), C.c_uint(uiBitsTemp), C.c_uint64(0)
            mvp = np.array(cMvPredBi[iRefList][iRefIdxTemp], np.int32)
            if D.bpref_me(p(blk), int(it["org_stride"]), px, py, w, h, iRefList, iRefIdxTemp, p(mvp), p(mv),
                          aaiMvpIdxBi[iRefList][iRefIdxTemp], C.byref(bits), C.byref(cost)):
                raise bc.RefThrows()
            cMvTemp[iRefList][iRefIdxTemp] = [int(mv[0]), int(mv[1])]
            before = aaiMvpIdxBi[iRefList][iRefIdxTemp]
            cMvPredBi[iRefList][iRefIdxTemp], aaiMvpIdxBi[iRefList][iRefIdxTemp], uiBitsTemp, uiCostTemp = check(
                iRefList, rec[iRefList][iRefIdxTemp], cMvTemp[iRefList][iRefIdxTemp], cMvPredBi[iRefList][iRefIdxTemp], before, bits.value, cost.value)
            if aaiMvpIdxBi[iRefList][iRefIdxTemp] != before:
                facts.add("mvp_switch")
            accepted = uiCostTemp < uiCostBi
            trace[calls] = (iRefList, iRefIdxTemp, [0, 0], cMvTemp[iRefList][iRefIdxTemp], uiBitsTemp, aaiMvpIdxBi[iRefList][iRefIdxTemp], int(accepted), 0, uiCostTemp)
            calls += 1
            if accepted:
                bChanged = True
                if iRefIdxTemp > 0:
                    facts.add("nonzero_ref_accepted")
                cMvBi[iRefList] = list(cMvTemp[iRefList][iRefIdxTemp])
                iRefIdxBi[iRefList] = iRefIdxTemp
                uiCostBi = uiCostTemp
                uiMotBits[iRefList] = uiBitsTemp - uiMbBits[2] - uiMotBits[1 - iRefList]
                uiBits2 = uiBitsTemp
                if num_iter != 1:
                    D.bpref_mc(px, py, w, h, iRefList, iRefIdxBi[iRefList], cMvBi[iRefList][0], cMvBi[iRefList][1], None)
        if not bChanged:
            if uiCostBi <= uiCost[0] and uiCostBi <= uiCost[1]:
                closing = 1
                # amvp[eRefPicList]: list 0's entry has just been overwritten with aacAMVPInfo[0][iRefIdxBi[0]] (:1146); list 1's still holds what the
                # loop above copied last (:1112), and gets aacAMVPInfo[1][iRefIdxBi[1]] only before the second call (:1154)
                amvp = rec[0][iRefIdxBi[0]] if iRefList == 0 else rec[1][n_ref[1] - 1]
                b0 = uiBits2
                r0 = iRefIdxBi[0]
                cMvPredBi[0][r0], aaiMvpIdxBi[0][r0], uiBits2, uiCostBi = check(0, amvp, cMvBi[0], cMvPredBi[0][r0], aaiMvpIdxBi[0][r0], uiBits2, uiCostBi)
                if not mvd_l1_zero:
                    amvp = rec[0][iRefIdxBi[0]] if iRefList == 0 else rec[1][iRefIdxBi[1]]
                    r1 = iRefIdxBi[1]
                    cMvPredBi[1][r1], aaiMvpIdxBi[1][r1], uiBits2, uiCostBi = check(1, amvp, cMvBi[1], cMvPredBi[1][r1], aaiMvpIdxBi[1][r1], uiBits2, uiCostBi)
                if uiBits2 != b0:
                    facts.add("closing_changes_bits")
            break
    res = np.zeros(1, abi.BIPRED_ME_RESULT)
    res[0] = (cMvBi, iRefIdxBi, [aaiMvpIdxBi[l][iRefIdxBi[l]] for l in range(2)], [cMvPredBi[l][iRefIdxBi[l]] for l in range(2)], uiBits2,
              [v & 0xFFFFFFFF for v in uiMotBits], calls, closing, 0, uiCostBi)
    return res[0], trace, facts


def build_items(rng, planes, org, bd, flags, fast, n_ref):
    """the candidate items of one group, with tags"""
    items, tags = [], []
    sad0 = 3 << (bd - 8)

    def rec_set(base, cands, spread=10, planes_of=None):
        return [[bc.ref_record(int(planes_of[l][r]) if planes_of else int(rng.integers(0, N_PLANES)), list(base + rng.integers(-spread, spread + 1, 2)), cands[l][r],
                               int(rng.integers(0, len(cands[l][r])))) for r in range(n_ref[l])] for l in range(2)]

    def add(tag, px, py, w, h, refs, cost_scale=(0.6, 1.6), org_off=None, ref_idx=None):
        ri = ref_idx if ref_idx is not None else [int(rng.integers(0, n_ref[0])), int(rng.integers(0, n_ref[1]))]
        cost = [int(w * h * sad0 * rng.uniform(*cost_scale)), int(w * h * sad0 * rng.uniform(*cost_scale))]
        items.append(bc.item(px, py, w, h, kit.sub_shift_of(w, h, fast), py * W + px if org_off is None else org_off, W, refs, ri, cost,
                             [int(rng.integers(8, 30)), int(rng.integers(8, 30))]))
        tags.append(tag)

    def shared(base, one=False):
        c = [list(base + rng.integers(-6, 7, 2))] if one else [list(base + rng.integers(-6, 7, 2)), list(base + rng.integers(-6, 7, 2))]
        return [[c] * n_ref[0], [c] * n_ref[1]]

    def place(w, h):
        return int(rng.integers(0, (W - 64 - w) // 4 + 1)) * 4 if w <= W - 64 else 0, int(rng.integers(0, (H - h) // 4 + 1)) * 4

    # every served shape: all references of an item share their candidates, so that the closing calls stay inside the contract
    for w in bc.SIDES:
        for h in bc.SIDES:
            px, py = place(w, h)
            base = rng.integers(-20, 21, 2)
            add("shape", px, py, w, h, rec_set(base, shared(base, one=(w + h) % 24 == 0)), (0.4, 3.0))
    # entries at the truth of an original that IS the mean of two displaced reference blocks: short runs
    for k in range(10):
        w, h = [(16, 16), (8, 8), (32, 16), (16, 32), (8, 16)][k % 5]
        px, py = 32 + 32 * (k % 5), 32 + 40 * (k // 5)
        pl = [[int(rng.integers(0, N_PLANES)) for _ in range(n_ref[l])] for l in range(2)]
        t = [rng.integers(-3, 4, 2), rng.integers(-3, 4, 2)]
        ri = [int(rng.integers(0, n_ref[0])), int(rng.integers(0, n_ref[1]))]
        b = [planes[pl[l][ri[l]]][py + t[l][1]:py + t[l][1] + h, px + t[l][0]:px + t[l][0] + w].astype(np.int32) for l in range(2)]
        org[py:py + h, px:px + w] = ((b[0] + b[1] + 1) >> 1).astype(np.int16)
        cands = shared(4 * t[0])
        refs = [[bc.ref_record(pl[l][r], list(4 * t[l] + (rng.integers(-2, 3, 2) if k >= 5 else 0)), cands[l][r], 0) for r in range(n_ref[l])] for l in range(2)]
        add("near", px, py, w, h, refs, (2.0, 3.0), ref_idx=ri)
    # all references share candidate 0 and start on it; candidate 1 differs per (list, reference): the closing calls see another set's candidate 1
    for k in range(14):
        w, h = [(16, 16), (8, 8), (32, 32), (16, 8)][k % 4]
        px, py = place(w, h)
        base = rng.integers(-12, 13, 2)
        c0 = list(base + rng.integers(-20, 21, 2))
        cands = [[[c0, list(base + rng.integers(-3, 4, 2)) if (l == 1 and r == n_ref[1] - 1) or k % 3 == 0 else list(base + rng.integers(60, 90, 2))]
                  for r in range(n_ref[l])] for l in range(2)]
        refs = [[bc.ref_record(int(rng.integers(0, N_PLANES)), list(base + rng.integers(-6, 7, 2)), cands[l][r], 0) for r in range(n_ref[l])] for l in range(2)]
        add("quirk", px, py, w, h, refs, (3.0, 4.0))
    # candidates of their own per (list, reference): the reference may throw in the closing calls
    for k in range(4):
        w, h = [(16, 16), (8, 8)][k % 2]
        px, py = place(w, h)
        base = rng.integers(-12, 13, 2)
        cands = [[[list(base + rng.integers(-6, 7, 2)), list(base + rng.integers(-6, 7, 2))] for r in range(n_ref[l])] for l in range(2)]
        add("own_sets", px, py, w, h, rec_set(base, cands), (0.5, 4.0))
    # picture corners, entry vectors far outside: clipMv binds on the vector and on the range
    z = np.zeros(2, np.int64)
    for (px, py, w, h, far) in [(0, 0, 32, 32, -4000), (W - 16, H - 16, 16, 16, 4000), (0, H - 8, 8, 8, -3000), (W - 64, 0, 64, 16, 5000)]:
        cands = shared(z)
        refs = [[bc.ref_record(int(rng.integers(0, N_PLANES)), [far + int(rng.integers(-40, 41)), (far if r % 2 == 0 else -far) + int(rng.integers(-40, 41))], cands[l][r], 0)
                 for r in range(n_ref[l])] for l in range(2)]
        add("corner", px, py, w, h, refs, (0.5, 50.0))
    # flat original
    fx, fy, _, _ = FLAT
    base = rng.integers(-8, 9, 2)
    add("flat", fx + 16, fy + 16, 16, 16, rec_set(base, shared(base)), (0.5, 3.0))
    add("flat", fx + 32, fy + 8, 8, 32, rec_set(base, shared(base)), (0.5, 3.0))
    return np.array(items, dtype=abi.BIPRED_ME_ITEM), tags


def build_set(D, bd, rng):
    mx = (1 << bd) - 1
    lam = 37.5 if bd == 10 else 11.25
    planes = np.stack([kit.texture(rng, H, W, bd, 1.5 * k) for k in range(N_PLANES)])
    org = np.clip(planes.astype(np.int32).mean(axis=0) + rng.integers(-5, 6, (H, W)), 0, mx).astype(np.int16)
    fx, fy, fw, fh = FLAT
    org[fy:fy + fh, fx:fx + fw] = mx // 3 + 7
    groups = [build_items(rng, planes, org, bd, flags, fast, n_ref) for flags, fast, n_ref in GROUPS]      # "near" items paint the original: all items first
    org = np.ascontiguousarray(org)
    cost = np.array(MVP_IDX_COST, np.uint32)
    items, group, want, trace, tags, facts = [], [], [], [], [], set()
    generated = dropped = 0
    for gi, ((flags, fast, n_ref), (its, tg)) in enumerate(zip(GROUPS, groups)):
        D.bpref_open(p(planes), N_PLANES, W, H, bd, C.c_double(lam), flags[3], flags[4], flags[5], fast, p(cost))
        for it, tag in zip(its, tg):
            generated += 1
            try:
                r, t, f = ref_loop(D, org, it, flags)
            except bc.RefThrows:
                dropped += 1
                continue
            items.append(it); group.append(gi); want.append(r); trace.append(t); tags.append(tag)
            facts |= f
    assert dropped * 4 <= generated, (dropped, generated)
    return (planes, org, np.array(items, dtype=abi.BIPRED_ME_ITEM), np.array(group, np.int32), lam, np.array(want, dtype=abi.BIPRED_ME_RESULT),
            np.array(trace, dtype=abi.BIPRED_ME_STEP), tags, facts, generated, dropped)


def check_set(bd, planes, org, items, group, lam, want, trace, tags, facts):
    """the restatement reproduces every reference result and trace entry (and supplies the integer vectors); the set holds the cases the tests rely on"""
    pp = kit.pad(planes)
    for gi, (flags, fast, n_ref) in enumerate(GROUPS):
        cfg = bc.cfg_dict(lam, W, H, bd, mvp_idx_cost=MVP_IDX_COST, **dict(zip(bc.GOLDEN_FLAGS, flags)))
        s = bc.Searcher(org, pp, cfg)
        for i in np.nonzero(group == gi)[0]:
            it = items[i]
            res, tr = s.search(it, strict=True)
            assert res.tobytes() == want[i].tobytes(), (bd, i, tags[i], res, want[i])
            got = tr.copy()
            got["int_mv"] = 0
            assert np.array_equal(got, trace[i]), (bd, i, tags[i], got, trace[i])
            trace[i] = tr
            n = int(res["me_calls"])
            w, h = int(it["w"]), int(it["h"])
            facts |= {("shape", w, h), ("n_ref", int(it["n_ref"][0])), ("n_ref", int(it["n_ref"][1])), ("range", flags[3]), ("num_iter", flags[0]),
                      ("pick", flags[1]), ("mvd_l1_zero", flags[2]), ("clip_key", flags[4]), ("hadamard", flags[5]), ("sub_shift", int(it["sub_shift"])),
                      ("passes", kit.passes(tr, n)), ("closing", int(res["closing"]))}
            if tags[i] == "corner":
                # clipMv binds on the vector (the first integer vector is the clipped entry's neighbourhood, far from the entry) and on the range
                e = it["ref"][int(tr[0]["list"])][int(tr[0]["ref"])]["mv"]
                assert abs(int(tr[0]["int_mv"][0]) * 4 - int(e[0])) > 4 * (flags[3] + 1), (bd, i)
                facts.add(("corner", int(it["pos_x"]) == 0))
            if tags[i] == "flat":
                facts.add("flat")
    need = [("shape", w, h) for w in bc.SIDES for h in bc.SIDES] + [("shape",) + s for s in NEEDED_SHAPES] + \
           [("n_ref", 1), ("n_ref", 2), ("n_ref", 4), ("range", 4), ("range", 2), ("num_iter", 4), ("num_iter", 1), ("pick", 1), ("pick", 0),
            ("mvd_l1_zero", 1), ("mvd_l1_zero", 0), ("clip_key", 1), ("clip_key", 0), ("hadamard", 1), ("hadamard", 0), ("sub_shift", 0), ("sub_shift", 1),
            ("passes", 1), ("passes", 2), ("passes", 3), ("passes", 4), ("closing", 0), ("closing", 1), "nonzero_ref_accepted", "mvp_switch",
            "closing_changes_bits", ("corner", True), ("corner", False), "flat"]
    for f in need:
        assert f in facts, (bd, f, sorted(map(str, facts)))


def main():
    D = driver()
    out = {}
    total = 0
    for bd in (10, 8):
        rng = np.random.default_rng(5200 + bd)
        planes, org, items, group, lam, want, trace, tags, facts, generated, dropped = build_set(D, bd, rng)
        check_set(bd, planes, org, items, group, lam, want, trace, tags, facts)
        k = "bd%d_" % bd
        out.update({k + "planes": planes, k + "org": org, k + "items": items, k + "group": group, k + "flags": np.array([g[0] for g in GROUPS], np.int32),
                    k + "lambda": np.float64(lam), k + "mvp_idx_cost": np.array(MVP_IDX_COST, np.uint32), k + "want": want, k + "trace": trace,
                    k + "dropped": np.int32(dropped), k + "generated": np.int32(generated)})
        total += len(items)
        ps = [kit.passes(trace[i], want[i]["me_calls"]) for i in range(len(items))]
        print("bit depth %d: %d items kept of %d (the reference throws on %d), passes %s, closing %d" % (bd, len(items), generated, dropped, np.bincount(ps), int(want["closing"].sum())))
    path = os.path.join(HERE, "bipred_me.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
