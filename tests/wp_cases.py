"""Explicit weighted prediction (vvcgpu_mc_wp_batch): the tests' restatement of the weighted epilogue and the helpers that build expected outputs.

P is the 14-bit intermediate of xPredInterBlk with rndRes = false -- what the MC checkers (oracle/_ref/libvtmref.so or the CPU restatement
oracle/liboracle.so, both `*_mc_batch`) store for bi = 2.  The restatement follows WeightPrediction.cpp:46-60 / 157-300:
  uni, w0 != 1 << shift   clip(((w0 (P0 + 8192) + (1 << (S - 1))) >> S) + offset)
  uni, w0 == 1 << shift   clip((((P0 + 8192) + (1 << (shiftNum - 1))) >> shiftNum) + offset)
  bi                      clip((w0 (P0 + 8192) + w1 (P1 + 8192) + (1 << (S - 1)) + (offset << (S - 1))) >> S)
with shiftNum = max(2, 14 - bd), S = shift + shiftNum.  tests/test_mc_wp_cpu.py pins it to tests/golden/wp.npz (the reference's own addWeightUni /
addWeightBi)."""
import numpy as np

from vvcsoftware_vtm_amd.abi import MC_DESC, WP_PARAM

IF_INTERNAL_OFFS = 8192


def apply(p0, p1, bi, e, bd, lo, hi):
    """the weighted epilogue on intermediates p0 (, p1): e = (w0, w1, offset, shift)"""
    w0, w1, offset, shift = (int(v) for v in e)
    shift_num = max(2, 14 - bd)
    s = shift + shift_num
    a0 = p0.astype(np.int64) + IF_INTERNAL_OFFS
    if bi:
        v = (w0 * a0 + w1 * (p1.astype(np.int64) + IF_INTERNAL_OFFS) + (1 << (s - 1)) + offset * (1 << (s - 1))) >> s
    elif w0 != 1 << shift:
        v = ((w0 * a0 + (1 << (s - 1))) >> s) + offset
    else:
        v = ((a0 + (1 << (shift_num - 1))) >> shift_num) + offset
    return np.clip(v, lo, hi).astype(np.int16)


def valid(e, bi, bd):
    """the range a WPScalingParam takes after getWpScaling; vvcgpu_mc_wp_batch skips a PU whose entry is outside it"""
    w0, w1, offset, shift = (int(v) for v in e)
    return abs(w0) <= 255 and (not bi or abs(w1) <= 255) and 0 <= shift <= 8 and abs(offset) <= 2 << bd


def intermediates(mc_batch, r0, r1, d, bd):
    """[(P0, P1 or None)] per descriptor: the bi = 2 predictions of list 0 from r0 (and of list 1 from r1 for bi = 1) through a checker's
    mc_batch(r0, r1, dst, descs, n, bd, lo, hi) (ctypes function of oraclelib.ref() or oraclelib.oracle())"""
    from oraclelib import p
    out = [[None, None] for _ in range(len(d))]
    for lst, plane in ((0, r0), (1, r1)):
        rows, where = [], []
        off = 0
        for i, r in enumerate(d):
            if lst == 1 and r["bi"] != 1:
                continue
            w, h = int(r["w"]), int(r["h"])
            q = np.zeros(1, MC_DESC)[0]
            q["ref0_off"], q["ref0_stride"] = (r["ref1_off"], r["ref1_stride"]) if lst else (r["ref0_off"], r["ref0_stride"])
            q["frac_x0"], q["frac_y0"] = (r["frac_x1"], r["frac_y1"]) if lst else (r["frac_x0"], r["frac_y0"])
            q["dst_off"], q["dst_stride"], q["w"], q["h"], q["is_luma"], q["bi"] = off, w, w, h, r["is_luma"], 2
            rows.append(q)
            where.append((i, off, w, h))
            off += w * h
        if not rows:
            continue
        qd = np.array(rows, MC_DESC)
        buf = np.zeros(off, np.int16)
        mc_batch(p(plane), p(plane), p(buf), p(qd), len(qd), bd, 0, (1 << bd) - 1)
        for i, o, w, h in where:
            out[i][lst] = buf[o:o + w * h].reshape(h, w)
    return [tuple(x) for x in out]


def expected(mc_batch, r0, r1, d, wp, bd, lo, hi, dst):
    """dst (a copy) after vvcgpu_mc_wp_batch of descriptors d with table wp: skipped descriptors leave their samples as they are"""
    dst = dst.copy()
    ok = [0 <= int(r["bi"]) <= 1 and 0 <= int(r["reserved"]) < len(wp) and 1 <= int(r["w"]) <= 128 and 1 <= int(r["h"]) <= 128
          and valid(wp[int(r["reserved"])], int(r["bi"]) == 1, bd) for r in d]
    take = d[np.array(ok, bool)] if len(d) else d
    for r, (p0, p1) in zip(take, intermediates(mc_batch, r0, r1, take, bd)):
        w, h, ds, o = int(r["w"]), int(r["h"]), int(r["dst_stride"]), int(r["dst_off"])
        v = apply(p0, p1, int(r["bi"]) == 1, wp[int(r["reserved"])], bd, lo, hi)
        for y in range(h):
            dst[o + y * ds:o + y * ds + w] = v[y]
    return dst


def table(records):
    return np.array(list(records), dtype=WP_PARAM)


def wp_sets(bd):
    """WP_PARAM records that cover the epilogue's branches: denominators 0 and 7, weights -128 / 0 / 255, w0 == 1 << shift with and without offset,
    negative and extreme offsets (up to the 2^(bd + 1) bound), bi with default and skewed weights; outputs clip at both ends on 'extreme' content"""
    sc = 1 << (bd - 8)
    top = 2 << bd
    uni = [(1, 0, 0, 0), (128, 0, 0, 7), (128, 0, -37 * sc, 7), (1, 0, 127 * sc, 0),                # w0 == 1 << shift
           (-128, 0, 5 * sc, 7), (255, 0, -128 * sc, 7), (0, 0, 64 * sc, 0), (255, 0, 127 * sc, 0),    # weighted
           (-128, 0, -128 * sc, 0), (3, 0, top, 1), (77, 0, -top, 5)]
    bi = [(1, 1, 0, 1), (128, 128, 0, 8), (-128, 255, 100 * sc, 8), (0, 255, -256 * sc, 1),          # shift = log2 denominator + 1
          (255, 255, top, 8), (-128, -128, -top, 1), (255, -128, 7, 3)]
    return uni, bi


def pu_list(rng, W, H, shapes, per, uni_idx, bi_idx, quarter=False, doff=0, margin=8):
    """descriptors (MC_DESC) of `per` PUs per (w, h, is_luma) shape with random positions in W x H planes and random phases (quarter: on the
    matrix-core grid), a full-sample PU among them; bi 0 / 1 alternate and take their table index from uni_idx / bi_idx in turn"""
    rows = []
    k = 0
    for (w, h, luma) in shapes:
        nf = 16 if luma else 32
        q = 4 if quarter else 1
        for i in range(per):
            bi = k & 1
            fr = [q * int(v) for v in rng.integers(0, nf // q, 4)]
            if i == 0:
                fr = [0, 0, 0, 0]
            x0, y0 = int(rng.integers(margin, W - w - margin)), int(rng.integers(margin, H - h - margin))
            x1, y1 = int(rng.integers(margin, W - w - margin)), int(rng.integers(margin, H - h - margin))
            ix = bi_idx[k % len(bi_idx)] if bi else uni_idx[k % len(uni_idx)]
            rows.append((y0 * W + x0, y1 * W + x1, doff, W, W, w, w, h, fr[0], fr[1], fr[2], fr[3], luma, bi, ix))
            doff += w * h
            k += 1
    return np.array(rows, MC_DESC), doff
