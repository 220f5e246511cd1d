"""Numpy restatement of the encoder picture analysis entries (vvcgpu_tile_stats_picture, vvcgpu_picture_sse, vvcgpu_picture_histogram,
vvcgpu_wp_sad_batch, vvcgpu_intra_cost_ctus) and of the two host finishers, plus the picture contents and candidate sets their tests share.
tests/golden/gen_analysis.py pins every function here to the compiled reference; the CPU and GPU tests compare the library against both."""
import math

import numpy as np

WP_HP, WP_CLIP = 1, 2                         # vvcgpu_wp_sad_cand.flags


# ---- picture contents -------------------------------------------------------------------------------------------------------------------------------
def content(rng, h, w, bd, kind):
    """noise; flat (activity below the lower limit of EncSlice.cpp:183 / EncGOP.cpp:2709); gradient; a black border frame around noise"""
    mx = (1 << bd) - 1
    if kind == "noise":
        return rng.integers(0, mx + 1, (h, w)).astype(np.int16)
    if kind == "flat":
        return (np.full((h, w), mx // 3) + rng.integers(0, 2, (h, w))).astype(np.int16)
    if kind == "gradient":
        yy, xx = np.mgrid[0:h, 0:w]
        return np.clip((xx * 3 + yy * 5) * mx // (3 * w + 5 * h) + rng.integers(-2, 3, (h, w)), 0, mx).astype(np.int16)
    if kind == "border":
        a = np.kron(rng.integers(mx // 4, mx + 1, (-(-h // 4), -(-w // 4))), np.ones((4, 4), np.int64))[:h, :w].astype(np.int16)     # 4 x 4 blocks of noise
        b = max(1, min(h, w) // 10)
        a[:b] = 0; a[-b:] = 0; a[:, :b] = 0; a[:, -b:] = 0
        return a
    raise ValueError(kind)


def distort(rng, org, bd, amp=6):
    """a 'reconstruction': the original plus small noise, clipped to the bit depth"""
    return np.clip(org.astype(np.int32) + rng.integers(-amp, amp + 1, org.shape), 0, (1 << bd) - 1).astype(np.int16)


# planes the golden fixture does not store: pure arithmetic on what it stores (no random stream to keep stable)
def rec_of(org, bd):
    """the fixture's 'reconstruction' of a plane: the original plus a small position pattern, clipped"""
    yy, xx = np.mgrid[0:org.shape[0], 0:org.shape[1]]
    return np.clip(org.astype(np.int32) + (xx * 7 + yy * 13) % 13 - 6, 0, (1 << bd) - 1).astype(np.int16)


def ref_of(org, bd):
    """the fixture's reference plane of the weighted SADs: the original faded (weight 54 / 64, offset 9 << (bd - 8)) plus a position pattern, clipped"""
    yy, xx = np.mgrid[0:org.shape[0], 0:org.shape[1]]
    return np.clip(((org.astype(np.int32) * 54 + 32) >> 6) + (9 << (bd - 8)) + (xx * 5 + yy * 3) % 7 - 3, 0, (1 << bd) - 1).astype(np.int16)


def big_plane(tile, h, w, bd):
    """a large plane from a small stored one: the tile repeated, plus a ramp down the rows, wrapped into the bit depth"""
    th, tw = tile.shape
    a = np.tile(tile.astype(np.int32), (-(-h // th), -(-w // tw)))[:h, :w]
    return ((a + (np.arange(h, dtype=np.int32) * 3)[:, None]) & ((1 << bd) - 1)).astype(np.int16)


# ---- tile statistics ------------------------------------------------------------------------------------------------------------------------------------
def highpass_abs(p):
    """|f| of the 3 x 3 high-pass filter at every sample that is not on the plane's outer row or column; 0 there"""
    a = p.astype(np.int64)
    out = np.zeros(a.shape, np.int64)
    if a.shape[0] < 3 or a.shape[1] < 3:
        return out
    c = a[1:-1, 1:-1]
    f = (12 * c - 2 * (a[1:-1, :-2] + a[1:-1, 2:] + a[:-2, 1:-1] + a[2:, 1:-1])
         - a[:-2, :-2] - a[:-2, 2:] - a[2:, :-2] - a[2:, 2:])
    out[1:-1, 1:-1] = np.abs(f)
    return out


def _tile_sums(v, t):
    h, w = v.shape
    ty, tx = -(-h // t), -(-w // t)
    pad = np.zeros((ty * t, tx * t), np.int64)
    pad[:h, :w] = v
    return pad.reshape(ty, t, tx, t).sum(axis=(1, 3))


def tile_stats(org, rec, t):
    """(tiles_y, tiles_x, 3) uint64: sa_act, sum, ss_err of the t x t tiles of one plane; rec may be None"""
    o = org.astype(np.int64)
    d = o - rec.astype(np.int64) if rec is not None else np.zeros_like(o)
    return np.stack([_tile_sums(highpass_abs(org), t), _tile_sums(o, t), _tile_sums(d * d, t)], axis=-1).astype(np.uint64)


def tile_area(h, w, t):
    """samples per tile, (tiles_y, tiles_x)"""
    return _tile_sums(np.ones((h, w), np.int64), t)


def tile_act_count(h, w, t):
    """filtered samples per tile = (iFltWidth - 2) * (iFltHeight - 2) of the reference's CTU loop = (wAct - xAct) * (hAct - yAct) of its WPSNR block"""
    m = np.zeros((h, w), np.int64)
    m[1:-1, 1:-1] = 1
    return _tile_sums(m, t)


def ctu_dc(stats, h, w, t):
    """m_iOffsetCtu per CTU from the tile sums (EncSlice.cpp:1437-1438)"""
    n = tile_area(h, w, t)
    return (stats[..., 1].astype(np.int64) + (n >> 1)) // n


def sse(a, b):
    d = a.astype(np.int64) - b.astype(np.int64)
    return int((d * d).sum())


# ---- WPSNR ------------------------------------------------------------------------------------------------------------------------------------------------------
def wpsnr_block_size(w, h, chroma_shift):
    """EncGOP.cpp:2741-2742 in the reference's types; 0 when the reference takes the plain SSE"""
    r = float((w * h) & 0xFFFFFFFF) / (1920.0 * 1080.0)
    b = min(128 >> chroma_shift, 4 * int(16.0 * math.sqrt(r) + 0.5))
    return b if b >= 4 else 0


def wpsnr_finish(stats, w, h, chroma_shift, bd):
    """EncGOP.cpp:2762-2794 on the tile statistics of the plane's own block size: the reference's operations in the reference's order"""
    b = wpsnr_block_size(w, h, chroma_shift)
    assert b >= 4
    s = np.asarray(stats).reshape(-1, 3)
    wmse, i = 0.0, 0
    for y in range(0, h, b):
        for x in range(0, w, b):
            bw, bh = min(b, w - x), min(b, h - y)
            x_act, y_act = (0 if x > 0 else 1), (0 if y > 0 else 1)
            h_act = bh if y + bh < h else bh - 1
            w_act = bw if x + bw < w else bw - 1
            sa, ss = int(s[i, 0]), int(s[i, 2])
            i += 1
            if w_act <= x_act or h_act <= y_act:
                wmse += float(ss)
                continue
            ms = float(sa) / (float(w_act - x_act) * float(h_act - y_act))
            if ms < float(1 << (bd - 4)):
                ms = float(1 << (bd - 4))
            ms *= ms
            wmse += float(ss) * math.pow(ms, -1.0 * 0.5)
    sum_act = 32.0 * float(1 << bd)
    if (w << chroma_shift) > 2048 and (h << chroma_shift) > 1280:
        sum_act *= 0.5
    elif (w << chroma_shift) <= 1024 or (h << chroma_shift) <= 640:
        sum_act *= 2.0
    return 0 if wmse <= 0.0 else int(wmse * math.pow(sum_act, 0.5) + 0.5)


def wpsnr_plane(org, rec, chroma_shift, bd):
    """xFindDistortionPlane(rec, org, rshift = bit depth, chromaShift): the plain SSE for planes too small for a WPSNR block"""
    h, w = org.shape
    b = wpsnr_block_size(w, h, chroma_shift)
    return sse(org, rec) if b == 0 else wpsnr_finish(tile_stats(org, rec, b), w, h, chroma_shift, bd)


def energy(sa_act, count, bd):
    """hpEner of filterAndCalculateAverageEnergies from its integers (EncSlice.cpp:180-183); count 0 (an area without interior) divides as the reference does"""
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.asarray(sa_act, np.float64) / np.asarray(count, np.float64)
    lim = float(1 << (bd - 4))
    return np.where(e < lim, lim, e)


# ---- weighted-prediction analysis ------------------------------------------------------------------------------------------------------------------------
def histogram(p, bd):
    return np.bincount(np.clip(p.astype(np.int64), 0, (1 << bd) - 1).reshape(-1), minlength=1 << bd).astype(np.uint32)


def _cdiv(a, b):
    """C's integer division (truncating)"""
    q = abs(a) // abs(b)
    return q if (a >= 0) == (b >= 0) else -q


def wp_acdc(hist, n_samples, fixed_shift):
    """(iDC, iAC) of xCalcACDCParamSlice (WeightPredAnalysis.cpp:267-297) from the histogram alone"""
    hh = [int(v) for v in hist]
    dc = sum(v * c for v, c in enumerate(hh))
    norm = _cdiv(dc + (n_samples >> 1), n_samples)
    ac = sum(c * abs(v - norm) for v, c in enumerate(hh))
    return _cdiv((dc << fixed_shift) + (n_samples >> 1), n_samples), ac


def wp_acdc_direct(p, fixed_shift):
    """the same from the samples, the reference's two passes"""
    a = p.astype(np.int64)
    n = a.size
    dc = int(a.sum())
    norm = _cdiv(dc + (n >> 1), n)
    return _cdiv((dc << fixed_shift) + (n >> 1), n), int(np.abs(a - norm).sum())


def wp_sad(org, ref, bd, cand):
    """one candidate (log2_denom, weight, offset, flags): xCalcSADvalueWP / xCalcSADvalueWPOptionalClip (WeightPredAnalysis.cpp:653-735)"""
    ld, wt, off, flags = (int(v) for v in cand)
    o, r = org.astype(np.int64), ref.astype(np.int64)
    hp = bool(flags & WP_HP)
    if flags & WP_CLIP:
        real = off << (0 if hp else bd - 8)
        rnd = 0 if ld == 0 else 1 << (ld - 1)
        sv = np.clip(((r * wt + rnd) >> ld) + real, 0, (1 << bd) - 1)
        return int(np.abs(o - sv).sum())
    real = off << (ld if hp else ld + bd - 8)
    return int(np.abs((o << ld) - (r * wt + real)).sum())


def wp_cands(bd):
    """16 candidates: default, typical and extreme weights and offsets, both precision flags, clipped and unclipped"""
    top = 1 << (bd - 1)
    c = [(0, 1, 0, 0), (6, 64, 0, 0), (6, 64, 0, WP_CLIP), (7, 128, 0, WP_HP),                       # default weights
         (6, 60, 3, 0), (6, 70, -5, WP_CLIP), (5, 29, 11, WP_HP), (5, 35, -17, WP_HP | WP_CLIP),      # typical
         (7, 255, -128, 0), (7, -128, 127, 0), (7, 255, 127, WP_CLIP), (7, -128, -128, WP_CLIP),      # extreme
         (7, 255, top - 1, WP_HP), (7, -127, -top, WP_HP), (0, 2, top - 1, WP_HP | WP_CLIP), (1, 1, -top, WP_HP | WP_CLIP)]
    return np.array(c, dtype=np.dtype([("log2_denom", "<i4"), ("weight", "<i4"), ("offset", "<i4"), ("flags", "<i4")]))


# ---- intra cost ---------------------------------------------------------------------------------------------------------------------------------------------
_H2 = np.array([[1, 1], [1, -1]], np.int64)
_H8 = np.kron(np.kron(_H2, _H2), _H2)


def intra_cost(org, ctu, bd):
    """(ctus_y, ctus_x) int32: (sumHad + offset) >> shift per CTU (EncSlice.cpp:1163-1204, EncCu.cpp:374-485)"""
    h, w = org.shape
    shift = bd - 8
    offset = 1 << (shift - 1) if shift > 0 else 0
    cy, cx = -(-h // ctu), -(-w // ctu)
    out = np.zeros((cy, cx), np.int32)
    a = org.astype(np.int64)
    for j in range(cy):
        for i in range(cx):
            blk = a[j * ctu:min((j + 1) * ctu, h), i * ctu:min((i + 1) * ctu, w)]
            bh, bw = blk.shape[0] // 8, blk.shape[1] // 8
            s = 0
            if bh and bw:
                b = blk[:bh * 8, :bw * 8].reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3)
                t = np.abs(_H8 @ b @ _H8)
                s = int((((t.sum(axis=(2, 3)) - t[..., 0, 0]) + 2) >> 2).sum())
            out[j, i] = (s + offset) >> shift
    return out


# ---- the shapes of the golden fixture ----------------------------------------------------------------------------------------------------------------
GOLDEN_PLANES = [(416, 240), (208, 120), (64, 64), (40, 24)]      # every content kind; 1920x1080 luma + 960x540 chroma: noise only
KINDS = ["noise", "flat", "gradient", "border"]
CTU_SIZES = [128, 64, 32]
INTRA_SIZES = [(416, 240), (200, 100), (139, 77), (64, 64), (40, 24)]    # ragged: the last 8 x 8 column / row is cut
