"""Generates tests/golden/intra_chroma_dq.npz: chroma PUs of the intra chroma mode loop under DepQuant 1 whose stored results come from the COMPILED
REFERENCE's own functions, through the wrappers oracle/_ref/libvtmref.so exports: vtmref_intra_pred (predIntraAng from unfiltered references) and, as the
chain steps of tests/rd_pass_kit.py call them, vtmref_pelop_area (AreaBuf::subtract), vtmref_tr_fwd_batch (xTrMxN_EMT), vtmref_depquant (DepQuant::quant; it
hands back the rate table it derived from its CABAC contexts), vtmref_dequant_tr_inv_batch with dep_quant = 1, vtmref_pelop (PelBufferOps reco) and
vtmref_dist (RdCost::xGetSSE).  LM predictions come from orc_cclm_pred, as in gen_intra_chroma_code.py.  Build machine only (needs oracle/_ref/libvtmref.so):
    python tests/golden/gen_intra_chroma_dq.py

vtmref_depquant builds Cb (or luma) TUs of an inter CU only, so the tables of the file are Cb tables for different (ctxQp, initId) pairs: the trellis is the
same function of a table whatever it was derived for.  The file therefore pins the arithmetic per item; the selection rule (record 1 or 2 of a PU by abs_sum
of the slot's Cb block) is applied here as include/vvcgpu.h states it from RateEstimator::xSetLastCoeffOffset, DeriveCtx::CtxQtCbf and
xRecurIntraChromaCodingQT, and is not captured from a run.  The generator asserts that the restatement (tests/intra_chroma_dq_cases.py) reproduces every
stored value and that the list meets golden_conditions.  Nothing of the reference is copied; only the data is stored."""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

import intra_chroma_code_cases as icc  # noqa: E402
import intra_chroma_dq_cases as cdq  # noqa: E402
import rd_pass_kit as kit  # noqa: E402
from oraclelib import p  # noqa: E402


def table(R, w, h, bd, qp, lam, ctx):
    """the rate table the reference derives for a Cb TU of this size under (ctxQp, initId)"""
    coef, level, rt = np.zeros(w * h, np.int32), np.zeros(w * h, np.int32), np.zeros(1, cdq.RATES)
    R.vtmref_depquant(p(coef), p(level), w, h, 1, bd, qp, C.c_double(lam), ctx[0], ctx[1], p(rt))
    return rt[0]


def ref_item(R, case, q, c, mode, refs, clp, j, ctx):
    """one (PU, slot, component) through the compiled reference with record j of the PU -> (pred, levels, abs_sum, rec, dist)"""
    cc = case.cc
    u, r = cc.pus[q], case.dq[3 * q + j]
    w, h, bd, qp = int(u["w"]), int(u["h"]), cc.bd, int(u["qp"][c])
    org = np.ascontiguousarray(kit.block(cc.org.reshape(-1), int(u["org_off"][c]), int(u["org_stride"]), w, h))
    if mode == icc.LM:
        pred = icc.predict(cc, q, c, mode, refs, clp)
    else:
        pred = np.zeros((h, w), np.int16)
        assert R.vtmref_intra_pred(p(refs), p(pred), w, w, h, mode, clp[0], clp[1], bd, 0, None) == 0
    coef, level, rt = kit.forward(kit.subtract(org, pred, bd, R), bd, 0, 0, R), np.zeros(w * h, np.int32), np.zeros(1, cdq.RATES)
    abs_sum = int(R.vtmref_depquant(p(coef), p(level), w, h, 1, bd, qp, C.c_double(float(r["lambda"])), ctx[0], ctx[1], p(rt)))
    assert rt[0].tobytes() == case.rates[int(r["rates_idx"])].tobytes()
    rec = kit.reconstruct(pred, kit.dequant_inverse(level, w, h, bd, 0, 0, qp, 1, R), clp, bd, R)
    return pred, level, abs_sum, rec, kit.sse(org, rec, bd, R)


def main():
    R = kit.reference()
    out = {}
    for bd in (8, 10):
        rng = np.random.default_rng(8900 + bd)
        clp = (0, (1 << bd) - 1)
        specs = cdq.golden_specs(bd)
        n = len(specs)
        case = cdq.make(rng, bd, specs, rates=np.zeros(3 * n, cdq.RATES))
        cc = case.cc
        case.dq["rates_idx"] = np.arange(3 * n)
        for q, u in enumerate(cc.pus):
            for j in range(3):
                case.rates[3 * q + j] = table(R, int(u["w"]), int(u["h"]), bd, int(u["qp"][min(j, 1)]), float(case.dq[3 * q + j]["lambda"]), cdq.golden_ctx(q)[j])
        flags = cdq.WRITE_PRED
        refs_b, pred_b, rec_b, level_b = cc.initial()
        abs_sum, dist = np.full((n, cdq.SLOTS, 2), cdq.U32_MAX, np.uint32), np.full((n, cdq.SLOTS, 2), cdq.U64_MAX, np.uint64)
        for q, u in enumerate(cc.pus):
            w, h = int(u["w"]), int(u["h"])
            for c in range(2):
                refs = icc.gathered(cc, q, c)
                refs_b[int(u["ref_off"][c]):int(u["ref_off"][c]) + refs.size] = refs
                for k in range(cdq.SLOTS):
                    mode = int(u["mode"][k])
                    if mode < 0:
                        continue
                    j = 0 if c == 0 else 2 if abs_sum[q, k, 0] > 0 else 1       # the selection rule, as the header states it
                    pred, level, abs_sum[q, k, c], rec, dist[q, k, c] = ref_item(R, case, q, c, mode, refs, clp, j, cdq.golden_ctx(q)[j])
                    co, lo = int(u["cand_off"]) + (2 * k + c) * w * h, int(u["level_off"]) + (2 * k + c) * w * h
                    pred_b[co:co + w * h], rec_b[co:co + w * h], level_b[lo:lo + w * h] = pred.reshape(-1), rec.reshape(-1), level
        want = cdq.restate(case, flags)
        kit.check_restatement(want, dict(refs=refs_b, pred=pred_b, rec=rec_b, level=level_b, abs_sum=abs_sum, dist=dist), bd)
        differ = cdq.golden_conditions(case, want)
        k = "bd%d_" % bd
        out.update({k + "luma": cc.luma, k + "rec": cc.rec, k + "org": cc.org, k + "avail": cc.avail, k + "pus": cc.pus.view(np.uint8),
                    k + "fill": cc.fill.view(np.uint8), k + "runs": cc.runs, k + "refs_size": np.int64(cc.refs_size), k + "cand_size": np.int64(cc.cand_size),
                    k + "level_size": np.int64(cc.level_size), k + "flags": np.int32(flags), k + "dq": case.dq.view(np.uint8), k + "rates": case.rates.view(np.int32),
                    k + "want_refs": refs_b, k + "want_pred": pred_b, k + "want_rec": rec_b, k + "want_level": level_b, k + "want_abs_sum": abs_sum, k + "want_dist": dist})
        print("bit depth %d: %d PUs, %d items, abs_sum == 0 in %d, Cr items that differ between the records %s" % (
            bd, n, int((abs_sum != cdq.U32_MAX).sum()), int((abs_sum == 0).sum()), differ))
    kit.save_golden(os.path.join(HERE, "intra_chroma_dq.npz"), out)


if __name__ == "__main__":
    main()
