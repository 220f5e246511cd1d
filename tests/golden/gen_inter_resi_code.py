"""Generates tests/golden/inter_resi_code.npz: items of the inter residual pixel pass (InterSearch::encodeResAndCalcRdInterCU, InterSearch.cpp:4752-4909, with
the "check full" part of xEstimateInterResidualQT, :4254-4634) whose every stored result comes from the COMPILED REFERENCE's own functions, through the
wrappers oracle/_ref/libvtmref.so exports, as the chain steps of tests/rd_pass_kit.py call them: vtmref_pelop_area (AreaBuf::subtract), vtmref_tr_fwd_batch (xTrMxN_EMT; tr_hor = 3: xTransformSkip),
vtmref_quant_batch (Quant::quant), vtmref_dequant_tr_inv_batch (Quant::dequant + xITrMxN_EMT or xITransformSkip), vtmref_pelop (PelBufferOps reco) and
vtmref_dist (RdCost::xGetSSE, on residual blocks and against a zero block as well).  Build machine only (needs oracle/_ref/libvtmref.so, i.e. a build()
where the reference exists):
    python tests/golden/gen_inter_resi_code.py

The tests' restatement (tests/inter_resi_code_cases.py) goes through the CPU restatement's steps; the generator asserts that it reproduces every stored value.
Nothing of the reference is copied; only the data is stored.  Inputs of the cases, not results of the reference: the planes, the predictions, the
transform candidates and the quantiser parameters."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

import inter_resi_code_cases as irc  # noqa: E402
import rd_pass_kit as kit  # noqa: E402

ROWS_H = 96                                                                  # rows of the original plane the file stores


def rows():
    """one row per shape class -> (w, h, slots, qp - 6 (bd - 8), intra_slice, sign_hiding): every shape with DCT-II; the four inter-EMT pairs on the squares
    4 .. 32 and some rectangles; transform skip on 4x4, 4x2 and 2x4; both slice types, sign hiding on and off, QPs 22 .. 37, the largest QP"""
    out = []
    qps = (22, 27, 32, 37, 24, 29, 35)
    for k, (w, h) in enumerate(irc.all_shapes()):
        tr = [0]
        if w == h and 4 <= w <= 32:
            tr += list(irc.EMT)
        elif 4 <= w <= 32 and 4 <= h <= 32 and k % 3 == 0:
            tr += [irc.EMT[k % 4], irc.EMT[(k + 1) % 4]]
        if (w, h) in ((4, 4), (4, 2), (2, 4)):
            tr.append(irc.TS)
        out.append((w, h, tr, qps[k % len(qps)], k % 2, (k // 2) % 2))
    out += [(16, 16, [0, 8], 63, 0, 1), (8, 8, [0, 4], 63, 1, 1), (4, 4, [0, irc.TS], 63, 0, 0), (64, 64, [0], 63, 0, 1), (4, 4, [irc.TS, 0], 22, 1, 1)]
    return out


def ref_item(R, case, i, clp):
    """one item through the compiled reference -> (zero_dist, [(k, levels, abs_sum, resi', rec, dist_resi, dist_rec)])"""
    it = case.items[i]
    w, h, bd = int(it["w"]), int(it["h"]), case.bd
    org = np.ascontiguousarray(irc.block(case.org, int(it["org_off"]), int(it["org_stride"]), w, h))
    pred = np.ascontiguousarray(irc.block(case.pred, int(it["pred_off"]), int(it["pred_stride"]), w, h))
    resi = kit.subtract(org, pred, bd, R)
    zero_dist = kit.sse(np.zeros((h, w), np.int16), resi, bd, R)
    slots = []
    for k in range(irc.SLOTS):
        code = int(it["tr"][k])
        if code < 0:
            continue
        th, tv = (3, 0) if code == irc.TS else (code % 3, code // 3)
        level, abs_sum, resi2 = kit.code_resi(resi, bd, th, tv, int(it["qp"]), int(it["intra_slice"]), int(it["sign_hiding"]), R)
        rec = kit.reconstruct(pred, resi2, clp, bd, R)
        slots.append((k, level, abs_sum, resi2, rec, kit.sse(resi, resi2, bd, R), kit.sse(org, rec, bd, R)))
    return zero_dist, slots


def main():
    R = kit.reference()
    out = {}
    for bd in (8, 10):
        rng = np.random.default_rng(8800 + bd)
        clp = (0, (1 << bd) - 1)
        plane = np.ascontiguousarray(irc.fresh_plane(rng, bd)[:ROWS_H])
        specs = []
        for q, (w, h, tr, qp, intra, sbh) in enumerate(rows()):
            x, _ = irc.place(rng, w, h, band=q % 3)
            specs.append(dict(x=x, y=int(rng.integers(0, ROWS_H - h + 1)), w=w, h=h, tr=tr, qp=qp + 6 * (bd - 8), intra=intra, sbh=sbh))
        case = irc.make(bd, plane, specs, rng)
        flags = irc.WRITE_REC
        want = irc.restate(case, flags)
        assert (want["abs_sum"] != irc.U32_MAX).sum() == sum(len(r[2]) for r in rows())          # every slot of the file is a served one
        resi_b, rec_b, level_b = case.initial()
        n = len(case.items)
        abs_sum = np.full((n, irc.SLOTS), irc.U32_MAX, np.uint32)
        dist_resi, dist_rec = np.full((n, irc.SLOTS), irc.U64_MAX, np.uint64), np.full((n, irc.SLOTS), irc.U64_MAX, np.uint64)
        zero_dist = np.zeros(n, np.uint64)
        for i, it in enumerate(case.items):
            sz = int(it["w"]) * int(it["h"])
            zero_dist[i], slots = ref_item(R, case, i, clp)
            for (k, level, asum, resi2, rec, dr, dc) in slots:
                co, lo = int(it["cand_off"]) + k * sz, int(it["level_off"]) + k * sz
                resi_b[co:co + sz], rec_b[co:co + sz], level_b[lo:lo + sz] = resi2.reshape(-1), rec.reshape(-1), level
                abs_sum[i, k], dist_resi[i, k], dist_rec[i, k] = asum, dr, dc
        kit.check_restatement(want, dict(resi=resi_b, rec=rec_b, level=level_b, abs_sum=abs_sum, dist_resi=dist_resi, dist_rec=dist_rec, zero_dist=zero_dist), bd)
        k = "bd%d_" % bd
        out.update({k + "org": case.org, k + "pred": case.pred, k + "items": case.items.view(np.uint8), k + "cand_size": np.int64(case.cand_size),
                    k + "level_size": np.int64(case.level_size), k + "flags": np.int32(flags), k + "want_resi": resi_b, k + "want_rec": rec_b,
                    k + "want_level": level_b, k + "want_abs_sum": abs_sum, k + "want_dist_resi": dist_resi, k + "want_dist_rec": dist_rec,
                    k + "want_zero_dist": zero_dist})
        served = abs_sum != irc.U32_MAX
        print("bit depth %d: %d items, %d slots, %d all-zero, the clip bites in %d" % (bd, n, served.sum(), (served & (abs_sum == 0)).sum(),
                                                                                    (served & (dist_rec != dist_resi)).sum()))
    kit.save_golden(os.path.join(HERE, "inter_resi_code.npz"), out)


if __name__ == "__main__":
    main()
