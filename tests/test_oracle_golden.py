"""CPU: the oracle restatement (oracle/restate) must reproduce every golden vector in tests/golden/*.npz, which were
produced by the COMPILED REFERENCE (tests/golden/gen_golden.py, gen_tr_tables.py).  This is what pins the oracle."""
import ctypes as C
import os

import numpy as np
import pytest

from oraclelib import oracle, p
from vvcsoftware_vtm_amd.abi import (AFFINE_PU, FRAC_BLK, FRAC_RESULT, MC_DESC, PELOP_DESC, RDPCM_DESC, SAO_DTYPE, DeblockCfg, MvCost,
                                     PelopCfg)

G = os.path.join(os.path.dirname(__file__), "golden")


def load(name):
    return np.load(os.path.join(G, name + ".npz"))


def test_alf_golden():
    g = load("alf")
    O = oracle()
    for ci in range(3):
        k = "c%d_" % ci
        w, h, ctu, bd = [int(v) for v in g[k + "meta"]]
        Y, Cb, Cr = g[k + "Y"], g[k + "Cb"], g[k + "Cr"]
        cls = np.zeros((h // 4, w // 4), np.uint16)
        O.orc_alf_classify(p(Y), w, w, h, bd, p(cls))
        assert np.array_equal(cls, g[k + "cls_all"])
        lc, cc = g[k + "lc"], g[k + "cc"]
        enY, enCb, enCr = g[k + "enY"], g[k + "enCb"], g[k + "enCr"]     # keep the arrays alive across the ctypes calls
        org = g[k + "org"] if (k + "org") in g.files else None
        mx = (1 << bd) - 1
        for ft in (0, 1):
            kk = "c%d_f%d_" % (ci, ft)
            dY, dCb, dCr = Y.copy(), Cb.copy(), Cr.copy()
            O.orc_alf_filter_luma(p(Y), w, p(dY), w, w, h, ctu, p(cls), ft, p(lc), p(enY), 0, mx)
            O.orc_alf_filter_chroma(p(Cb), w // 2, p(dCb), w // 2, w // 2, h // 2, ctu // 2, p(cc), p(enCb), 0, mx)
            O.orc_alf_filter_chroma(p(Cr), w // 2, p(dCr), w // 2, w // 2, h // 2, ctu // 2, p(cc), p(enCr), 0, mx)
            assert np.array_equal(dY, g[kk + "dY"]) and np.array_equal(dCb, g[kk + "dCb"]) and np.array_equal(dCr, g[kk + "dCr"])
            if (k + "stats_f%d" % ft) in g.files:
                want = g[k + "stats_f%d" % ft]
                got = np.zeros_like(want)
                O.orc_alf_stats(p(org), w, p(Y), w, w, h, ctu, p(cls), ft, p(got))
                assert np.array_equal(got, want)


def test_sao_golden():
    g = load("sao")
    O = oracle()
    for ci in range(3):
        k = "c%d_" % ci
        w, h, cw, bd = [int(v) for v in g[k + "meta"]]
        Y = g[k + "Y"]
        prm = g[k + "prm"].view(SAO_DTYPE)
        d = Y.copy()
        O.orc_sao_apply(p(Y), w, p(d), w, w, h, cw, cw, bd, p(prm), 0, (1 << bd) - 1)
        assert np.array_equal(d, g[k + "out"])
        st = np.zeros_like(g[k + "stats"])
        org = g[k + "org"]
        O.orc_sao_stats(p(org), w, p(Y), w, w, h, cw, cw, bd, None, 5, 4, p(st))
        assert np.array_equal(st, g[k + "stats"])


def test_dist_golden():
    g = load("dist")
    O = oracle()
    for f in ("orc_sad", "orc_satd", "orc_sse", "orc_mvcost", "orc_mrsad", "orc_mrsatd"):
        getattr(O, f).restype = C.c_uint64
    W = g["org10"].shape[1]
    for row in g["rows"]:
        bd, kind, ox, oy, cx, cy, w, h, ss, want = [int(v) for v in row]
        org, cur = g["org%d" % bd], g["cur%d" % bd]
        po = C.c_void_p(org.ctypes.data + 2 * (oy * W + ox))
        pc = C.c_void_p(cur.ctypes.data + 2 * (cy * W + cx))
        got = (O.orc_sad(po, W, pc, W, w, h, ss) if kind == 0 else O.orc_satd(po, W, pc, W, w, h) if kind == 1 else O.orc_sse(po, W, pc, W, w, h) if kind == 2
               else O.orc_mrsad(po, W, pc, W, w, h, ss) if kind == 3 else O.orc_mrsatd(po, W, pc, W, w, h))
        assert got == want, (bd, kind, w, h, ss)
    assert {int(r[1]) for r in g["rows"]} == {0, 1, 2, 3, 4}
    for r in g["mvcost"]:
        m = MvCost(float(r[0]), int(r[1]), int(r[2]), int(r[3]), int(r[4]))
        assert O.orc_mvcost(C.byref(m), int(r[5]), int(r[6])) == int(r[7])


def test_interp_golden():
    g = load("interp")
    O = oracle()
    for bd in (8, 10):
        mx = (1 << bd) - 1
        ref_ = g["ref%d" % bd]
        W = ref_.shape[1]
        rows, off, want = g["pred_rows%d" % bd], g["pred_off%d" % bd], g["pred_out%d" % bd]
        for (x, y, w, h, luma, fx, fy, rnd, i) in rows:
            d = np.zeros((h, w), np.int16)
            m = np.array([(y * W + x, 0, 0, W, W, w, w, h, fx, fy, 0, 0, luma, 0 if rnd else 2, 0)], MC_DESC)
            O.orc_mc_batch(p(ref_), p(ref_), p(d), p(m), 1, bd, 0, mx)
            assert np.array_equal(d.reshape(-1), want[off[i]:off[i + 1]]), (bd, x, y, w, h, luma, fx, fy, rnd)
        inter = g["inter%d" % bd]
        pos = 0
        for r in g["if_rows%d" % bd]:
            x, y, w, h, N, isV, isF, isL = [int(v) for v in r[:8]]
            cf = r[8:].astype(np.int16)
            src = ref_ if isF else inter
            d = np.zeros((h, w), np.int16)
            O.orc_if_filter(N, isV, isF, isL, C.c_void_p(src.ctypes.data + 2 * (y * W + x)), W, p(d), w, w, h, p(cf), bd, 0, mx)
            assert np.array_equal(d.reshape(-1), g["if_out%d" % bd][pos:pos + w * h]), (bd, w, h, N, isV, isF, isL)
            pos += w * h


def test_transform_golden():
    g = load("transform")
    O = oracle()
    for bd in (8, 10):
        pos = 0
        for (w, h, th, tv) in g["rows%d" % bd]:
            w, h, th, tv = int(w), int(h), int(th), int(tv)
            n = w * h
            r = g["resi%d" % bd][pos:pos + n].copy()
            want = g["coef%d" % bd][pos:pos + n]
            c = np.zeros(n, np.int32)
            O.orc_tr_fwd(p(r), w, p(c), w, h, th, tv, bd)
            assert np.array_equal(c, want), (bd, w, h, th, tv)
            q = ((want >> 4) << 4).astype(np.int32)
            ri = np.zeros(n, np.int16)
            O.orc_tr_inv(p(q), p(ri), w, w, h, th, tv, bd)
            assert np.array_equal(ri, g["inv%d" % bd][pos:pos + n]), (bd, w, h, th, tv)
            pos += n


def test_transform_worst_golden():
    """restatement == compiled reference at the exactness bounds of the device transforms (tests/golden/gen_golden.py:gen_transform_worst): residuals
    aligned with a basis row at the full amplitude, full-scale coefficients aligned with one output sample; the inputs are rebuilt from the rows"""
    import cases
    g = dict(load("transform_worst"))                       # (decompressed once)
    assert np.array_equal(g["rows"], cases.tr_worst_rows()) and np.array_equal(g["inv_rows"], cases.tr_worst_inv_rows())
    O = oracle()
    pos = 0
    for row in g["rows"]:
        w, h, th, tv, k, l, negate, amp, bd = (int(v) for v in row)
        r = np.ascontiguousarray(cases.tr_aligned_block(w, h, th, tv, k, l, amp, bool(negate)))
        c = np.zeros(w * h, np.int32)
        O.orc_tr_fwd(p(r), w, p(c), w, h, th, tv, bd)
        assert np.array_equal(c, g["coef"][pos:pos + w * h]), tuple(row)
        pos += w * h
    assert pos == g["coef"].size
    pos = 0
    for row in g["inv_rows"]:
        w, h, th, tv, x, y, val, bd = (int(v) for v in row)
        q = np.ascontiguousarray(cases.tr_aligned_coeffs(w, h, th, tv, x, y, val))
        ri = np.zeros(w * h, np.int16)
        O.orc_tr_inv(p(q), p(ri), w, w, h, th, tv, bd)
        assert np.array_equal(ri, g["inv"][pos:pos + w * h]), tuple(row)
        pos += w * h
    assert pos == g["inv"].size


def test_transform_skip_golden():
    """T3 pinned: restatement == TrQuant::xTransformSkip / xITransformSkip of the compiled reference."""
    g = load("tskip")
    O = oracle()
    for bd in (8, 10):
        pos = 0
        for (w, h) in g["rows%d" % bd]:
            w, h = int(w), int(h)
            n = w * h
            r = g["resi%d" % bd][pos:pos + n].copy()
            c = np.zeros(n, np.int32)
            O.orc_tr_fwd(p(r), w, p(c), w, h, 3, 0, bd)
            assert np.array_equal(c, g["coef%d" % bd][pos:pos + n]), (bd, w, h)
            q = g["cin%d" % bd][pos:pos + n].copy()
            ri = np.zeros(n, np.int16)
            O.orc_tr_inv(p(q), p(ri), w, w, h, 3, 0, bd)
            assert np.array_equal(ri, g["inv%d" % bd][pos:pos + n]), (bd, w, h)
            pos += n


def test_dequant_golden():
    """N1 pinned: scans, Quant::dequant and the dependent-quantisation state machine == the compiled reference."""
    g = load("dequant")
    O = oracle()
    pos = 0
    for w in (2, 4, 8, 16, 32, 64):
        for h in (2, 4, 8, 16, 32, 64):
            sc = np.zeros(w * h, np.uint32)
            O.orc_scan_order(w, h, p(sc))
            assert np.array_equal(sc.astype(np.uint16), g["scan"][pos:pos + w * h]), (w, h)
            pos += w * h
    for bd in (8, 10):
        pos = 0
        for (w, h, qp, dq) in g["rows%d" % bd]:
            w, h, qp, dq = int(w), int(h), int(qp), int(dq)
            n = w * h
            lv = g["level%d" % bd][pos:pos + n].copy()
            o = np.zeros(n, np.int32)
            O.orc_dequant(dq, bd, qp, 0, p(lv), p(o), w, h)
            assert np.array_equal(o, g["coef%d" % bd][pos:pos + n]), (bd, w, h, qp, dq)
            pos += n


def test_affine_gradient_golden():
    """N3 pinned: restatement == the compiled reference's SIMD table slots (Sobel planes, equal-coefficient sums)."""
    g = load("affine")
    O = oracle()
    pos = 0
    for n, (w, h) in enumerate(g["rows"]):
        w, h = int(w), int(h)
        cnt = w * h
        pred = g["pred"][pos:pos + cnt].copy()
        gx = np.zeros(cnt, np.int32); gy = np.zeros(cnt, np.int32)
        O.orc_affine_sobel(0, p(pred), w, p(gx), w, w, h)
        O.orc_affine_sobel(1, p(pred), w, p(gy), w, w, h)
        assert np.array_equal(gx, g["gx"][pos:pos + cnt]) and np.array_equal(gy, g["gy"][pos:pos + cnt]), (w, h)
        resi = g["resi"][pos:pos + cnt].copy()
        for six in (0, 1):
            eq = np.zeros(49, np.int64)
            O.orc_affine_equal_coeff(p(resi), p(gx), p(gy), w, w, h, six, p(eq))
            assert np.array_equal(eq, g["eq"][(2 * n + six) * 49:(2 * n + six + 1) * 49]), (w, h, six)
        pos += cnt


def test_frac_refine_golden():
    g = load("frac")
    O = oracle()
    for bd in (8, 10):
        ref_, org = g["ref%d" % bd], g["org%d" % bd]
        W = org.shape[1]
        for r in g["rows%d" % bd]:
            _, w, h, had, ph, pv = [int(v) for v in r[:6]]
            blk = np.array([tuple(int(v) for v in r[6:12])], FRAC_BLK)
            want = tuple(int(v) for v in r[12:18])
            m = MvCost(float(r[18]), ph, pv, 0, 0)
            res = np.zeros(1, FRAC_RESULT)
            O.orc_frac_refine(p(org), W, p(ref_), ref_.shape[1], p(blk), 1, w, h, bd, 0, (1 << bd) - 1, had, C.byref(m), p(res))
            assert tuple(int(res[0][k]) for k in FRAC_RESULT.names) == want, (bd, w, h, had)


def test_transform_tables_golden_and_shipped():
    """restated initROM formulas == tables dumped from the compiled reference == table compiled into the HIP library."""
    from vvcsoftware_vtm_amd import capi
    O = oracle()
    O.orc_tr_matrix.restype = C.POINTER(C.c_int16)
    lib = capi.lib()
    g = load("tr_tables")
    for t, nm in enumerate(["DCT2", "DCT8", "DST7"]):
        for lg in range(1, 7):
            N = 1 << lg
            want = g["%s_%d" % (nm, N)]
            a = np.ctypeslib.as_array(O.orc_tr_matrix(t, N), shape=(N * N,)).reshape(N, N)
            b = np.ctypeslib.as_array(C.cast(lib.vvcgpu_tr_matrix_host(t, N), C.POINTER(C.c_int16)), shape=(N * N,)).reshape(N, N)
            assert np.array_equal(a, want) and np.array_equal(b, want)
            # the identities the reference's 4-point fast forms rely on (TrQuant_EMT.cpp:1654-1662)
            if N == 4 and t == 2:
                assert want[0][0] + want[0][1] == want[0][3]


def test_tz_search_golden():
    """next row N2: restated xTZSearch vs the compiled reference's own InterSearch::xTZSearch (position, cost, SAD)."""
    g = load("tzsearch")
    import cases
    O = oracle()
    moved = 0
    for k in range(2):
        org, ref_, bd = g["org%d" % k], g["ref%d" % k], int(g["bd%d" % k])
        for j in range(3):
            pus, cfg, want = g["pus%d_%d" % (k, j)], g["cfg%d_%d" % (k, j)], g["res%d_%d" % (k, j)]
            assert pus.dtype == cases.TZ_PU and cfg.dtype == cases.TZ_CFG
            got = np.zeros(len(pus), cases.BEST)
            pus, cfg = np.ascontiguousarray(pus), np.ascontiguousarray(cfg)
            O.orc_tz_search(p(org), org.shape[1], p(ref_), ref_.shape[1], p(pus), len(pus), p(cfg), p(got))
            assert np.array_equal(got, want), (k, j, np.nonzero(got != want)[0][:5])
            moved += int(np.sum((want["x"] != 0) | (want["y"] != 0)))
    assert moved > 100      # the fixture's searches really leave the zero vector


def test_picture_passes_golden():
    """next row N4: restated extendPicBorder / compCRC / compChecksum vs the compiled reference (Picture::extendPicBorder on a real
    Picture: the fixture generator asserted that its output is the edge-replicated input, and stores digests of it)."""
    g = load("picture")
    O = oracle()
    for k in range(4):
        w, h, bd, margin = [int(v) for v in g["meta%d" % k]]
        for c in range(3):
            pl = np.ascontiguousarray(g["in%d_%d" % (k, c)])
            m = margin >> (c > 0)
            buf = np.full((pl.shape[0] + 2 * m, pl.shape[1] + 2 * m), -7, np.int16)
            buf[m:m + pl.shape[0], m:m + pl.shape[1]] = pl
            O.orc_extend_border(C.c_void_p(buf.ctypes.data + (m * buf.shape[1] + m) * 2), buf.shape[1], pl.shape[1], pl.shape[0], m, m)
            assert np.array_equal(buf, np.pad(pl, m, mode="edge"))
            b64 = buf.astype(np.int64)
            assert [int(b64.sum()), int((b64 * np.arange(buf.size).reshape(buf.shape) % 65521).sum())] == [int(v) for v in g["padsum%d_%d" % (k, c)]]
            assert (O.orc_crc(bd, p(pl), pl.shape[1], pl.shape[1], pl.shape[0]) & 0xffffffff) == int(g["crc%d_%d" % (k, c)])
            assert (O.orc_checksum(bd, p(pl), pl.shape[1], pl.shape[1], pl.shape[0]) & 0xffffffff) == int(g["sum%d_%d" % (k, c)])


def test_intra_pred_golden():
    """next row N4: restated predIntraAng (planar / DC / angular incl. wide angles, PDPC, reference filter) vs the compiled reference."""
    g = load("intra")
    O = oracle()
    refs_all, pred_all = g["refs"], g["pred"]
    seen = set()
    for (w, h, mode, bd, filt, T, L, ro, po) in g["rows"]:
        t, l = C.c_int(), C.c_int()
        O.orc_intra_ref_lengths(int(w), int(h), C.byref(t), C.byref(l))
        assert (t.value, l.value) == (T, L)
        refs = np.ascontiguousarray(refs_all[ro:ro + T + L + 1])
        if filt:
            f = np.zeros_like(refs)
            O.orc_intra_filter_refs(p(refs), p(f), int(w), int(h))
            refs = f
        pred = np.zeros((h, w), np.int16)
        O.orc_intra_pred(p(refs), p(pred), int(w), int(w), int(h), int(mode), 0, (1 << int(bd)) - 1)
        assert np.array_equal(pred.reshape(-1), pred_all[po:po + w * h]), (w, h, mode, bd, filt)
        seen.add(int(mode))
    assert seen == set(range(67))


def cclm_records():
    g = load("cclm")
    hdr, win, nb, pred = g["hdr"], g["win"], g["nb"], g["pred"]
    wo = no = po = 0
    for (w, h, above, left, bdl, bdc, cmin, cmax, lw, lh) in hdr:
        yield (int(w), int(h), int(above), int(left), int(bdl), int(bdc), int(cmin), int(cmax), int(lw), int(lh),
               np.ascontiguousarray(win[wo:wo + lw * lh]), np.ascontiguousarray(nb[no:no + w + h]), pred[po:po + w * h])
        wo += lw * lh; no += w + h; po += w * h


def test_cclm_golden():
    """next row N4, CCLM: restated xGetLumaRecPixels + xGetLMParameters + predIntraChromaLM vs blocks captured from the reference's own
    predIntraChromaLM inside reference encoder runs (tests/golden/gen_cclm.py)."""
    O = oracle()
    n = 0
    combos = set()
    for (w, h, above, left, bdl, bdc, cmin, cmax, lw, lh, win, nb, want) in cclm_records():
        got = np.zeros((h, w), np.int16)
        origin = C.c_void_p(win.ctypes.data + (2 * lw + 3) * 2)
        O.orc_cclm_pred(origin, lw, p(nb), C.c_void_p(nb.ctypes.data + 2 * w), p(got), w, w, h, above, left, bdl, bdc, cmin, cmax)
        assert np.array_equal(got.reshape(-1), want), (w, h, above, left, bdc)
        n += 1
        combos.add((w, h, above, left))
    assert n > 500 and len(combos) > 50


def intra_fill_records():
    g = load("intra_fill")
    hdr, flags, top, left, out = g["hdr"], g["flags"], g["top"], g["left"], g["out"]
    fo = to = lo = oo = 0
    for (w, h, uw, uh, bd, T, L, total) in hdr:
        w, h, uw, uh, bd, T, L, total = [int(v) for v in (w, h, uw, uh, bd, T, L, total)]
        topN, leftN = 1 + ((T + uw - 1) // uw) * uw, ((L + uh - 1) // uh) * uh
        # rebuild a small reconstruction plane: row 0 = the row above (from x = -1), column 0 = the column to the left
        plane = np.zeros((leftN + 1, topN), np.int16)
        plane[0, :] = top[to:to + topN]
        plane[1:, 0] = left[lo:lo + leftN]
        yield w, h, uw, uh, bd, T, L, np.ascontiguousarray(flags[fo:fo + total]), plane, out[oo:oo + T + L + 1]
        fo += total; to += topN; lo += leftN; oo += T + L + 1


def test_intra_fill_refs_golden():
    """next row N4: restated xFillReferenceSamples vs samples captured from the reference's own function inside encoder runs
    (tests/golden/gen_intra_fill.py): 1584 calls, most of them with partially available neighbours."""
    O = oracle()
    n = partial = 0
    for (w, h, uw, uh, bd, T, L, flags, plane, want) in intra_fill_records():
        got = np.zeros(T + L + 1, np.int16)
        O.orc_intra_fill_refs(C.c_void_p(plane.ctypes.data + (plane.shape[1] + 1) * 2), plane.shape[1], p(flags), p(got), w, h, uw, uh, bd)
        assert np.array_equal(got, want), (w, h, uw, uh, flags.tolist())
        n += 1
        partial += 0 < int(flags.sum()) < len(flags)
    assert n > 1000 and partial > 500


def test_imv_refine_golden():
    """next row N2 (AMVR): restated xPatternSearchIntRefine vs the compiled reference's own function."""
    import cases
    g = load("imv")
    O = oracle()
    org, ref_ = g["org"], g["ref"]
    for j in range(4):
        pus, cfg, want = np.ascontiguousarray(g["pus%d" % j]), np.ascontiguousarray(g["cfg%d" % j]), g["res%d" % j]
        sh, had, wgt = g["par%d" % j]
        got = np.zeros(len(pus), cases.IMV_RESULT)
        O.orc_imv_refine(p(org), org.shape[1], p(ref_), ref_.shape[1], p(pus), len(pus), p(cfg), int(had), C.c_double(float(wgt)), p(got))
        assert np.array_equal(got, want), (j, np.nonzero(got != want)[0][:5])


def test_quant_golden():
    """next row N1, forward: restated Quant::quant (+ sign bit hiding) vs the compiled reference."""
    g = load("quant")
    O = oracle()
    O.orc_quant.restype = C.c_uint32
    hidden = 0
    for (w, h, bd, qp, intra, sbh, off, s) in g["rows"]:
        n = int(w * h)
        coef = np.ascontiguousarray(g["coef"][off:off + n])
        lv = np.zeros(n, np.int32)
        assert O.orc_quant(p(coef), p(lv), int(w), int(h), int(bd), int(qp), int(intra), int(sbh)) == int(s)
        assert np.array_equal(lv, g["level"][off:off + n]), (w, h, bd, qp, intra, sbh)
        if sbh:
            plain = np.zeros(n, np.int32)
            O.orc_quant(p(coef), p(plain), int(w), int(h), int(bd), int(qp), int(intra), 0)
            hidden += int(np.any(plain != lv))
    assert hidden > 30          # the fixture really exercises the hiding adjustment


def depquant_rows():
    g = load("depquant")
    for r in g["rows"]:
        w, h, comp, bd, qp, off, s, ri = [int(v) for v in r[:8]]
        yield w, h, comp, bd, qp, off, s, ri, float(r[8]), g


def test_depquant_golden():
    """next row N1: the restated dependent-quantisation trellis vs the compiled reference's own DepQuant::quant."""
    O = oracle()
    O.orc_depquant.restype = C.c_uint32
    n = nz = 0
    for (w, h, comp, bd, qp, off, s, ri, lam, g) in depquant_rows():
        coef = np.ascontiguousarray(g["coef"][off:off + w * h])
        rt = np.ascontiguousarray(g["rates"][ri:ri + 1])
        lv = np.zeros(w * h, np.int32)
        assert O.orc_depquant(p(coef), p(lv), w, h, 1 - comp, bd, qp, C.c_double(lam), p(rt)) == s
        assert np.array_equal(lv, g["level"][off:off + w * h]), (w, h, comp, bd, qp)
        n += 1
        nz += int(np.count_nonzero(lv))
    assert n > 80 and nz > 5000


def rdoq_rows():
    g = load("rdoq")
    for r in g["rows"]:
        w, h, comp, bd, qp, off, s, ri = [int(v) for v in r[:8]]
        yield w, h, comp, bd, qp, off, s, ri, float(r[8]), int(r[9]), g


def test_rdoq_golden():
    """next row N1: the restated rate-distortion optimised quantiser vs the compiled reference's own QuantRDOQ::quant."""
    O = oracle()
    O.orc_rdoq.restype = C.c_uint32
    n = nz = changed = 0
    for (w, h, comp, bd, qp, off, s, ri, lam, sbh, g) in rdoq_rows():
        coef = np.ascontiguousarray(g["coef"][off:off + w * h])
        rt = np.ascontiguousarray(g["rates"][ri:ri + 1])
        lv = np.full(w * h, 77, np.int32)
        assert O.orc_rdoq(p(coef), p(lv), w, h, 1 - comp, bd, qp, C.c_double(lam), sbh, p(rt)) == s, (w, h, comp, bd, qp)
        assert np.array_equal(lv, g["level"][off:off + w * h]), (w, h, comp, bd, qp)
        n += 1
        nz += int(np.count_nonzero(lv))
        if sbh:
            plain = np.zeros(w * h, np.int32)
            O.orc_rdoq(p(coef), p(plain), w, h, 1 - comp, bd, qp, C.c_double(lam), 0, p(rt))
            changed += int(np.any(plain != lv))
    assert n > 100 and nz > 5000 and changed > 20          # the fixture exercises the sign-hiding adjustment too


def test_rdpcm_golden():
    """oracle/restate/rdpcm.cpp == TrQuant::applyForwardRDPCM / invRdpcmNxN of the compiled reference (tests/golden/rdpcm.npz)"""
    g = np.load(os.path.join(G, "rdpcm.npz"))
    rows = g["rows"]
    offs = np.concatenate([[0], np.cumsum(rows[:, 1] * rows[:, 2])])
    for i, (bd, w, h, mode, lossless, rot, intra, qp) in enumerate(rows):
        d = np.zeros(1, RDPCM_DESC); d[0] = (0, 0, w, w, h, mode, lossless, rot, intra, qp, 0, 0)
        resi = np.ascontiguousarray(g["resi"][offs[i]:offs[i + 1]])
        c = np.zeros(w * h, np.int32); sm = np.zeros(1, np.uint32)
        oracle().orc_rdpcm_fwd_batch(p(resi), p(c), p(d), 1, int(bd), p(sm))
        assert np.array_equal(c, g["coef"][offs[i]:offs[i + 1]]) and sm[0] == g["abs_sum"][i], rows[i]
        if rot == 0:
            a = np.ascontiguousarray(g["inv_in"][offs[i]:offs[i + 1]])
            oracle().orc_rdpcm_inv_batch(p(a), p(d), 1)
            assert np.array_equal(a, g["inv_out"][offs[i]:offs[i + 1]]), rows[i]


def test_affine_subblock_vectors_golden():
    """oracle/restate/rdpcm.cpp:orc_affine_subblock_descs + the (pinned) block interpolation == InterPrediction::xPredAffineBlk of the compiled
    reference on 120 PUs x 3 components (tests/golden/affine_mv.npz)"""
    g = np.load(os.path.join(G, "affine_mv.npz"))
    W, H, bd, M = 256, 128, 10, 144
    pads = [np.ascontiguousarray(np.pad(g[k], M >> (1 if c else 0), mode="edge")) for c, k in enumerate(("Y", "Cb", "Cr"))]
    o = 0
    for r in g["rows"]:
        px, py, w, h, six = [int(v) for v in r[:5]]
        for comp in range(3):
            c = 1 if comp else 0
            mv = np.zeros((2, 3, 2), np.int32); mv[0] = r[5:11].reshape(3, 2)
            pu = np.zeros(1, AFFINE_PU); pu[0] = (px, py, w, h, six, 0, mv, 0, w >> c, 0)
            nd = (w // 4) * (h // 4)
            d = np.zeros(nd, MC_DESC)
            oracle().orc_affine_subblock_descs(p(pu), 1, c, W, H, 128, 128, M >> c, M >> c, pads[comp].shape[1], pads[comp].shape[1], p(d))
            got = np.zeros((h >> c) * (w >> c), np.int16)
            oracle().orc_mc_batch(p(pads[comp]), p(pads[comp]), p(got), p(d), nd, bd, 0, 1023)
            n = got.size
            assert np.array_equal(got, g["pred"][o:o + n]), (r.tolist(), comp)
            o += n



def test_deblock_golden():
    """L1 + L2: the restatement (oracle/restate/deblock.cpp) on the planes in front of the compiled reference's LoopFilter::loopFilterPic, with the
    (edge, BS) / QP maps recorded from the reference's own xDeblockCU walk, equals the planes behind the reference's own sample filters
    (LoopFilter.cpp:149-230, 543-980; fixture: tests/golden/gen_deblock.py) -- inter pictures with affine 4x4 sub-block edges and CUs beyond 64
    samples (transform-edge splits), and a 1920x1080 dual-tree intra picture with non-zero beta / tc / chroma QP offsets."""
    import cases
    pics = cases.deblock_golden()
    assert len(pics) == 3
    assert pics[0]["hdr"]["n_affine"] > 50 and pics[1]["hdr"]["n_cu_gt64"] > 8 and pics[2]["hdr"]["w"] == 1920 and pics[2]["hdr"]["dual_tree"] == 1
    for r in pics:
        h = r["hdr"]
        cfg = DeblockCfg(h["bd_luma"], h["bd_chroma"], h["beta_offset_div2"], h["tc_offset_div2"], h["cb_qp_offset"], h["cr_qp_offset"],
                         (C.c_int32 * 3)(h["clp_min0"], h["clp_min1"], h["clp_min2"]), (C.c_int32 * 3)(h["clp_max0"], h["clp_max1"], h["clp_max2"]))
        Y, Cb, Cr = (x.copy() for x in r["pre"])
        oracle().orc_deblock(p(Y), h["w"], p(Cb), p(Cr), h["w"] // 2, h["w"], h["h"], p(r["ev"]), p(r["eh"]), p(r["qp_luma"]), p(r["qp_chroma"]), C.byref(cfg))
        assert not np.array_equal(Y, r["pre"][0])
        for got, want, name in zip((Y, Cb, Cr), r["post"], "Y Cb Cr".split()):
            assert np.array_equal(got, want), "poc %d %s: %d samples differ" % (h["poc"], name, int((got != want).sum()))


def pelop_cases(g, bd):
    """(op, source planes, one-descriptor list, config, expected block) per row of tests/golden/pelop.npz"""
    W = g["pel%d" % bd].shape[1]
    src = {0: ("inter", "inter"), 1: ("pel", "resi"), 2: ("pel", "pel"), 3: ("pel", "pel"), 4: ("pel", "pel"), 5: ("resi", "resi")}
    exp = g["out%d" % bd]
    for (op, w, h, bd_, clip, scale, shift, offset, cmin, cmax, x0, y0, x1, y1, pos) in g["rows%d" % bd]:
        a, b = (g[n + str(bd)] for n in src[int(op)])
        d = np.array([(y0 * W + x0, y1 * W + x1, 0, W, W, w, w, h)], dtype=PELOP_DESC)
        yield int(op), a, b, d, PelopCfg(int(scale), int(shift), int(offset), int(clip), int(cmin), int(cmax)), exp[pos:pos + w * h]


def test_pelop_golden():
    """B1-B4: orc_pelop_batch == the reference's PelBufferOps table (addAvg / reco / linTf) and AreaBuf subtract / removeHighFreq / copyClip."""
    g = load("pelop")
    O = oracle()
    n = 0
    for bd in (8, 10):
        for op, a, b, d, cfg, want in pelop_cases(g, bd):
            got = np.full(want.size, -77, np.int16)
            O.orc_pelop_batch(op, p(a), p(b), p(got), p(d), 1, C.byref(cfg))
            assert np.array_equal(got, want), (op, bd, d)
            n += 1
    assert n > 500
