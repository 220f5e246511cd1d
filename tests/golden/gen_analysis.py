"""Generates tests/golden/analysis.npz: encoder picture analysis by the COMPILED REFERENCE.  Build machine only (needs the reference tree and
oracle/_ref/libvtmref.so, i.e. a build() where the reference exists):  python tests/golden/gen_analysis.py

gen_analysis_driver.cpp is compiled here against the reference where it lies and linked with libvtmref.so; nothing of the reference is copied, only
the resulting data is stored.  What is the reference's own code: EncGOP::xFindDistortionPlane (plain SSE and both WPSNR chroma shifts),
filterAndCalculateAverageEnergies, xCalcSADvalueWP, xCalcSADvalueWPOptionalClip, xCalcHistogram, WeightPredAnalysis::xCalcACDCParamSlice (through a
Slice whose Picture carries an original buffer) and EncCu::updateCtuDataISlice.  What is restated HERE because the reference has it inline in a
function that needs a whole encoder: the CTU and fltArea rectangles and the DC rounding of EncSlice::compressSlice (EncSlice.cpp:1412-1438), and the
clipped CTU rectangle, shift and offset of EncSlice::calCostSliceI (:1172-1199).

Stored per bit depth (8, 10), plane size (416x240, 208x120, 64x64, 40x24) and content (noise, flat, gradient, border): the plane and the
reference's outputs.  The reconstruction, the reference plane of the weighted SADs and the 1920x1080 / 960x540 planes are arithmetic on stored planes
(analysis_cases.rec_of / ref_of / big_plane), so the fixture stays small.  The restatement of tests/analysis_cases.py is asserted equal to every
reference output here, the floating-point finals included (libm's pow is the one of the machine that built the reference)."""
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

import analysis_cases as ac  # noqa: E402
from oraclelib import p  # noqa: E402

REF = os.environ.get("REF", "/root/reference")


def driver():
    src = os.path.join(REF, "source", "Lib")
    inc = ["-I" + os.path.join(src, d) for d in ("", "CommonLib", "CommonLib/x86", "libmd5", "EncoderLib", "DecoderLib", "Utilities")]
    refdir = os.path.join(ROOT, "oracle", "_ref")
    out = os.path.join(tempfile.mkdtemp(), "libanaref.so")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-fPIC", "-shared", "-msse4.1", "-w", "-DNDEBUG", "-fno-access-control"] + inc +
                          [os.path.join(HERE, "gen_analysis_driver.cpp"), "-o", out, "-L" + refdir, "-lvtmref", "-Wl,-rpath," + refdir])
    d = C.CDLL(out)
    d.anaref_dist_plane.restype = C.c_uint64
    d.anaref_energy.restype = C.c_double
    d.anaref_wp_sad.restype = C.c_int64
    return d


def qpa_ctus(D, org, t, bd):
    """hpEner and DC per CTU with the rectangles of EncSlice.cpp:1412-1420"""
    h, w = org.shape
    ty, tx = -(-h // t), -(-w // t)
    ener, dc = np.zeros((ty, tx), np.float64), np.zeros((ty, tx), np.int64)
    for j in range(ty):
        for i in range(tx):
            x, y = i * t, j * t
            sw, sh = min(t, w - x), min(t, h - y)                                   # subArea
            fx, fy = (x - 1 if x > 0 else 0), (y - 1 if y > 0 else 0)               # fltArea, clipped to the picture
            fw, fh = min(t + (2 if x > 0 else 1), w - fx), min(t + (2 if y > 0 else 1), h - fy)
            ener[j, i] = D.anaref_energy(p(org[fy:, fx:]), org.strides[0] // 2, fh, fw, bd)
            s = int(org[y:y + sh, x:x + sw].astype(np.int64).sum())
            n = sh * sw
            dc[j, i] = (s + (n >> 1)) // n
    return ener, dc


def plane_outputs(D, org, bd, out, k):
    """the reference's outputs of one plane under the key prefix k; asserts the restatement equal to each"""
    h, w = org.shape
    st = org.strides[0] // 2
    rec, ref = ac.rec_of(org, bd), ac.ref_of(org, bd)
    # plain SSE and WPSNR, the plane taken as luma (chroma shift 0) and as chroma (1)
    out[k + "sse"] = np.uint64(D.anaref_dist_plane(p(rec), w, p(org), st, w, h, 0, 0))
    assert int(out[k + "sse"]) == ac.sse(org, rec)
    for cs in (0, 1):
        v = D.anaref_dist_plane(p(rec), w, p(org), st, w, h, bd, cs)
        assert v == ac.wpsnr_plane(org, rec, cs, bd), (k, cs, v, ac.wpsnr_plane(org, rec, cs, bd))
        out[k + "wpsnr_cs%d" % cs] = np.uint64(v)
    # perceptual QP adaptation: whole plane, and per CTU
    e = D.anaref_energy(p(org), st, h, w, bd)
    whole = ac.tile_stats(org, None, 128)
    assert e == float(ac.energy(int(whole[..., 0].sum()), (w - 2) * (h - 2), bd)), k
    out[k + "plane_ener"] = np.float64(e)
    for t in ac.CTU_SIZES:
        ener, dc = qpa_ctus(D, org, t, bd)
        s = ac.tile_stats(org, None, t)
        assert np.array_equal(ener, ac.energy(s[..., 0], ac.tile_act_count(h, w, t), bd)), (k, t)
        assert np.array_equal(dc, ac.ctu_dc(s, h, w, t)), (k, t)
        assert int(s[..., 0].sum()) == int(whole[..., 0].sum())
        out[k + "qpa%d_ener" % t], out[k + "qpa%d_dc" % t] = ener, dc.astype(np.int32)
    # weighted-prediction analysis
    hist = np.zeros(1 << bd, np.int32)
    D.anaref_histogram(p(org), w, h, st, 1 << bd, p(hist))
    assert np.array_equal(hist.astype(np.uint32), ac.histogram(org, bd)), k
    out[k + "hist"] = hist
    cands = ac.wp_cands(bd)
    sad = np.zeros(len(cands), np.int64)
    for i, c in enumerate(cands):
        ld, wt, off, fl = (int(v) for v in c)
        sad[i] = D.anaref_wp_sad(bd, p(org), p(ref), w, h, st, w, ld, wt, off, fl & 1, 1, (fl >> 1) & 1)
        if not fl & 2:
            assert sad[i] == D.anaref_wp_sad(bd, p(org), p(ref), w, h, st, w, ld, wt, off, fl & 1, 0, 0)
        assert sad[i] == ac.wp_sad(org, ref, bd, c), (k, i)
    out[k + "wp_sad"] = sad


def intra_outputs(D, org, ctu, bd):
    h, w = org.shape
    shift = bd - 8
    offset = 1 << (shift - 1) if shift > 0 else 0
    cy, cx = -(-h // ctu), -(-w // ctu)
    cost = np.zeros((cy, cx), np.int32)
    for j in range(cy):
        for i in range(cx):
            x, y = i * ctu, j * ctu
            s = D.anaref_ctu_sum_had(p(org[y:, x:]), org.strides[0] // 2, min(ctu, w - x), min(ctu, h - y))
            cost[j, i] = (s + offset) >> shift
    assert np.array_equal(cost, ac.intra_cost(org, ctu, bd)), (org.shape, ctu, bd)
    return cost


def main():
    D = driver()
    out = {}
    for bd in (8, 10):
        rng = np.random.default_rng(900 + bd)
        planes = {}
        for (w, h) in ac.GOLDEN_PLANES:
            for kind in ac.KINDS:
                org = ac.content(rng, h, w, bd, kind)
                planes[(w, h, kind)] = org
                k = "bd%d_%dx%d_%s_" % (bd, w, h, kind)
                out[k + "org"] = org
                plane_outputs(D, org, bd, out, k)
        # the large set: not stored, rebuilt from the 64x64 noise plane
        for (w, h) in ((1920, 1080), (960, 540)):
            org = ac.big_plane(planes[(64, 64, "noise")], h, w, bd)
            plane_outputs(D, org, bd, out, "bd%d_%dx%d_big_" % (bd, w, h))
        # AC / DC of a picture: Y 416x240, Cb 208x120 of the same content, Cr 208x120 of the next one; both settings of the high-precision flag
        for i, kind in enumerate(ac.KINDS):
            y, cb, cr = planes[(416, 240, kind)], planes[(208, 120, kind)], planes[(208, 120, ac.KINDS[(i + 1) % 4])]
            acdc = np.zeros((2, 6), np.int64)
            for hp in (0, 1):
                D.anaref_acdc(p(y), p(cb), p(cr), 416, 240, hp, p(acdc[hp]))
                for c, pl in enumerate((y, cb, cr)):
                    want = ac.wp_acdc(ac.histogram(pl, bd), pl.size, 0)
                    assert want == ac.wp_acdc_direct(pl, 0) == (int(acdc[hp, 2 * c]), int(acdc[hp, 2 * c + 1])), (bd, kind, hp, c)
            out["bd%d_acdc_%s" % (bd, kind)] = acdc
        # intra cost: crops of the 416x240 planes (ragged sizes cut the last 8 x 8 column / row)
        for (w, h) in ac.INTRA_SIZES:
            for kind in ("noise", "gradient"):
                org = np.ascontiguousarray(planes[(416, 240, kind)][:h, :w])
                for ctu in (128, 64):
                    out["bd%d_intra_%dx%d_%s_ctu%d" % (bd, w, h, kind, ctu)] = intra_outputs(D, org, ctu, bd)
    path = os.path.join(HERE, "analysis.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
