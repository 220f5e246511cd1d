"""Generates tests/golden/intra_tu_dq.npz: items of the intra RD loop's pixel pass under DepQuant 1 (IntraSearch::xIntraCodingTUBlock, IntraSearch.cpp:1147-1316,
with transformNxN / invTransformNxN going through DQIntern::DepQuant) whose every stored result comes from the COMPILED REFERENCE's own functions, through the
wrappers oracle/_ref/libvtmref.so exports: vtmref_intra_pred (predIntraAng with xFilterReferenceSamples in front) and, as the chain steps of
tests/rd_pass_kit.py call them, vtmref_pelop_area (AreaBuf::subtract), vtmref_tr_fwd_batch (xTrMxN_EMT), vtmref_depquant (DepQuant::quant; it hands back the rate
table it derived from its CABAC contexts), vtmref_dequant_tr_inv_batch with dep_quant = 1 (DepQuant::dequant + xITrMxN_EMT), vtmref_pelop (PelBufferOps reco)
and vtmref_dist (RdCost::xGetSSE).  Build machine only (needs oracle/_ref/libvtmref.so, i.e. a build() where the reference exists):
    python tests/golden/gen_intra_tu_dq.py

The tests' restatement (tests/intra_tu_dq_cases.py) goes through the CPU restatement's steps; the generator asserts that it reproduces every stored value.
Nothing of the reference is copied; only the data is stored.  Inputs of the cases, not results of the reference: the planes, the modes, the filter decisions,
the given predictions, the transform pairs, the QPs, the lambdas, the (ctxQp, initId) pairs the rate tables are derived for, and the packed references
(gathered by orc_intra_fill_refs, which tests/golden/intra_fill.npz checks against the reference's own calls).  The reference wrapper derives its tables for a
CU of its own making, so a luma table's cbf bits are the wrapper's choice; the trellis is the same function of the table whichever CU it was filled for."""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

import intra_mode_cand_cases as imc  # noqa: E402
import intra_tu_code_cases as itc  # noqa: E402
import intra_tu_dq_cases as tdq  # noqa: E402
import rd_pass_kit as kit  # noqa: E402
from oraclelib import p  # noqa: E402


def rows():
    """one row per item -> (w, h, mode (-1: a given prediction), tr_hor, tr_ver, qp - 6 (bd - 8), comp): all 25 shapes with DCT-II; the four EMT pairs on the
    squares 4 .. 32 and two on some rectangles; luma and Cb tables; QPs 22 .. 37, the largest QP; two given predictions"""
    out = []
    qps = (22, 27, 32, 37, 24, 29, 35)
    for k, (w, h) in enumerate(imc.all_shapes()):
        comp = 1 if max(w, h) <= 32 and k % 2 else 0
        out.append((w, h, itc.MODES[k % len(itc.MODES)], 0, 0, qps[k % len(qps)], comp))
        if w == h and w <= 32:
            out += [(w, h, itc.MODES[(k + 3 * a + b) % len(itc.MODES)], a, b, qps[(k + a + 2 * b) % len(qps)], (a + b + k) % 2) for a in (1, 2) for b in (1, 2)]
        elif w <= 32 and h <= 32 and k % 3 == 0:
            out += [(w, h, 50 if w > h else 18, 1 + k % 2, 2 - k % 2, 27, 0), (w, h, 3 if w > h else 65, 2, 2, 22, 1)]
    out += [(16, 16, 1, 0, 0, 63, 0), (8, 8, 34, 2, 1, 63, 1), (4, 4, 0, 0, 0, 63, 0), (64, 64, 66, 0, 0, 63, 0), (16, 16, -1, 0, 0, 27, 0), (8, 8, -1, 2, 2, 22, 1)]
    return out


def ref_item(R, case, i, clp, comp, cq, init):
    """one item through the compiled reference -> (pred, levels, abs_sum, rec, dist, the rate table)"""
    tc = case.tc
    it, q = tc.items[i], case.dq[i]
    u = tc.base.pus[int(it["pu"])]
    w, h, bd, mode, th, tv = int(it["w"]), int(it["h"]), tc.bd, int(it["mode"]), int(it["tr_hor"]), int(it["tr_ver"])
    org = np.ascontiguousarray(tc.base.org[int(u["y"]):int(u["y"]) + h, int(u["x"]):int(u["x"]) + w])
    if mode == itc.PRED_GIVEN:
        pred = itc.block(tc.pred0, int(it["pred_off"]), int(it["pred_stride"]), w, h).copy()
    else:
        pred = np.zeros((h, w), np.int16)
        assert R.vtmref_intra_pred(p(tc.refs_of(int(it["pu"]))), p(pred), w, w, h, mode, clp[0], clp[1], bd, int(it["filt"]), None) == 0
    coef, level, rt = kit.forward(kit.subtract(org, pred, bd, R), bd, th, tv, R), np.zeros(w * h, np.int32), np.zeros(1, tdq.RATES)
    abs_sum = int(R.vtmref_depquant(p(coef), p(level), w, h, comp, bd, int(it["qp"]), C.c_double(float(q["lambda"])), cq, init, p(rt)))
    rec = kit.reconstruct(pred, kit.dequant_inverse(level, w, h, bd, th, tv, int(it["qp"]), 1, R), clp, bd, R)
    return pred, level, abs_sum, rec, kit.sse(org, rec, bd, R), rt[0]


def main():
    R = kit.reference()
    out = {}
    for bd in (8, 10):
        rng = np.random.default_rng(9800 + bd)
        clp = (0, (1 << bd) - 1)
        base = itc.fresh_base(rng, bd, [(r[0], r[1]) for r in rows()])
        specs, ctx = [], []
        for q, (w, h, mode, th, tv, qp, comp) in enumerate(rows()):
            f = int(imc.use_filtered(w, h, mode)) if q % 4 and mode >= 0 else q % 8 // 4
            # lambda and the context state the rate table is derived for: as gen_inter_resi_dq.py
            specs.append(dict(pu=q, mode=mode, filt=f, tr_hor=th, tr_ver=tv, qp=qp + 6 * (bd - 8), luma=1 - comp, lam=float(rng.uniform(5, 400)), rates_idx=q))
            ctx.append((comp, int(rng.integers(20, 45)), int(rng.integers(0, 3))))
        n = len(specs)
        case = tdq.make(base, specs, rng, rates=np.zeros(n, tdq.RATES))
        tc = case.tc
        flags = itc.WRITE_PRED
        assert {int(v) for v in tc.items["filt"][tc.items["mode"] >= 0]} == {0, 1} and (tc.items["mode"] == itc.PRED_GIVEN).sum() == 2
        pred_b, rec_b, level_b = tc.initial()
        abs_sum, num_sig, dist = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint64)
        for i, it in enumerate(tc.items):
            w, h = int(it["w"]), int(it["h"])
            pred, level, abs_sum[i], rec, dist[i], case.rates[i] = ref_item(R, case, i, clp, *ctx[i])
            num_sig[i] = np.count_nonzero(level)
            itc.block(pred_b, int(it["pred_off"]), int(it["pred_stride"]), w, h)[:] = pred
            itc.block(rec_b, int(it["rec_off"]), int(it["rec_stride"]), w, h)[:] = rec
            level_b[int(it["level_off"]):int(it["level_off"]) + w * h] = level
        want = tdq.restate(case, flags)
        kit.check_restatement(want, dict(pred=pred_b, rec=rec_b, level=level_b, abs_sum=abs_sum, num_sig=num_sig, dist=dist), bd)
        assert (want["abs_sum"] != tdq.U32_MAX).all()                        # every item of the file is a served one
        assert (abs_sum > 0).sum() * 3 >= n and (abs_sum == 0).any()         # levels, and the early return
        assert len({case.rates[i].tobytes() for i in range(n)}) >= 4
        k = "bd%d_" % bd
        out.update({k + "rec": base.rec, k + "org": base.org, k + "pus": base.pus.view(np.uint8), k + "avail": base.avail, k + "items": tc.items.view(np.uint8),
                    k + "dq": case.dq.view(np.uint8), k + "rates": case.rates.view(np.int32),
                    k + "pred0": tc.pred0, k + "rec_size": np.int64(tc.rec_size), k + "level_size": np.int64(tc.level_size), k + "flags": np.int32(flags),
                    k + "want_pred": pred_b, k + "want_rec": rec_b, k + "want_level": level_b, k + "want_abs_sum": abs_sum, k + "want_num_sig": num_sig,
                    k + "want_dist": dist})
        print("bit depth %d: %d items, %d all-zero, %d distinct rate tables, num_sig %s" % (
            bd, n, (abs_sum == 0).sum(), len({case.rates[i].tobytes() for i in range(n)}), [int(v) for v in num_sig]))
    kit.save_golden(os.path.join(HERE, "intra_tu_dq.npz"), out)


if __name__ == "__main__":
    main()
