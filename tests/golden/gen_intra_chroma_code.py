"""Generates tests/golden/intra_chroma_code.npz: chroma PUs of the intra chroma mode loop (IntraSearch::estIntraPredChromaQT, IntraSearch.cpp:704-852) whose
stored results come from the COMPILED REFERENCE's own functions, through the wrappers oracle/_ref/libvtmref.so exports: vtmref_intra_pred (predIntraAng from
unfiltered references, 2-sample sides included) and, as the chain steps of tests/rd_pass_kit.py call them, vtmref_pelop_area (AreaBuf::subtract), vtmref_tr_fwd_batch (xTrMxN_EMT), vtmref_quant_batch (Quant::quant),
vtmref_dequant_tr_inv_batch (Quant::dequant + xITrMxN_EMT), vtmref_pelop (PelBufferOps reco) and vtmref_dist (RdCost::xGetSSE).  Build machine only (needs
oracle/_ref/libvtmref.so, i.e. a build() where the reference exists):
    python tests/golden/gen_intra_chroma_code.py

The LM predictions come from orc_cclm_pred: xGetLMParameters takes the availability of the neighbours from a walk over the encoder's coding structure
(isAboveAvailable / isLeftAvailable over cs.getCURestricted), which does not exist outside an encoder run; orc_cclm_pred is pinned by tests/golden/cclm.npz,
the inputs and outputs of the reference's own predIntraChromaLM calls captured inside encoder runs (docs/ORACLE.md).
The tests' restatement (tests/intra_chroma_code_cases.py) goes through the CPU restatement's steps; the generator asserts that it reproduces every stored
value -- which also proves the restated predIntraAng on 2-sample sides.  Nothing of the reference is copied; only the data is stored.  Inputs of the cases,
not results of the reference: the modes, the quantiser parameters, the availability flags, and the packed references (gathered by orc_intra_fill_refs, which
tests/golden/intra_fill.npz checks against the reference's own calls)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

import intra_chroma_code_cases as icc  # noqa: E402
import rd_pass_kit as kit  # noqa: E402
from oraclelib import p  # noqa: E402


def ref_item(R, case, q, c, mode, refs, clp):
    """one (PU, slot, component) through the compiled reference -> (pred, levels, abs_sum, rec, dist)"""
    u = case.pus[q]
    w, h, bd, qp = int(u["w"]), int(u["h"]), case.bd, int(u["qp"][c])
    org = np.ascontiguousarray(kit.block(case.org.reshape(-1), int(u["org_off"][c]), int(u["org_stride"]), w, h))
    if mode == icc.LM:
        pred = icc.predict(case, q, c, mode, refs, clp)
    else:
        pred = np.zeros((h, w), np.int16)
        assert R.vtmref_intra_pred(p(refs), p(pred), w, w, h, mode, clp[0], clp[1], bd, 0, None) == 0
    level, abs_sum, resi2 = kit.code_resi(kit.subtract(org, pred, bd, R), bd, 0, 0, qp, int(u["intra_slice"]), int(u["sign_hiding"]), R)
    rec = kit.reconstruct(pred, resi2, clp, bd, R)
    return pred, level, abs_sum, rec, kit.sse(org, rec, bd, R)


def main():
    R = kit.reference()
    out = {}
    for bd in (8, 10):
        rng = np.random.default_rng(8800 + bd)
        clp = (0, (1 << bd) - 1)
        case = icc.make(rng, bd, icc.golden_specs(bd))
        flags = icc.WRITE_PRED
        want = icc.restate(case, flags)
        icc.conditions(case, want)
        refs_b, pred_b, rec_b, level_b = case.initial()
        n = len(case.pus)
        abs_sum, dist = np.full((n, icc.SLOTS, 2), icc.U32_MAX, np.uint32), np.full((n, icc.SLOTS, 2), icc.U64_MAX, np.uint64)
        for q, u in enumerate(case.pus):
            w, h = int(u["w"]), int(u["h"])
            for c in range(2):
                refs = icc.gathered(case, q, c)
                refs_b[int(u["ref_off"][c]):int(u["ref_off"][c]) + refs.size] = refs
                for k in range(icc.SLOTS):
                    mode = int(u["mode"][k])
                    if mode < 0:
                        continue
                    pred, level, abs_sum[q, k, c], rec, dist[q, k, c] = ref_item(R, case, q, c, mode, refs, clp)
                    co, lo = int(u["cand_off"]) + (2 * k + c) * w * h, int(u["level_off"]) + (2 * k + c) * w * h
                    pred_b[co:co + w * h], rec_b[co:co + w * h], level_b[lo:lo + w * h] = pred.reshape(-1), rec.reshape(-1), level
        kit.check_restatement(want, dict(refs=refs_b, pred=pred_b, rec=rec_b, level=level_b, abs_sum=abs_sum, dist=dist), bd)
        k = "bd%d_" % bd
        out.update({k + "luma": case.luma, k + "rec": case.rec, k + "org": case.org, k + "avail": case.avail, k + "pus": case.pus.view(np.uint8),
                    k + "fill": case.fill.view(np.uint8), k + "runs": case.runs, k + "refs_size": np.int64(case.refs_size), k + "cand_size": np.int64(case.cand_size),
                    k + "level_size": np.int64(case.level_size), k + "flags": np.int32(flags), k + "want_refs": refs_b, k + "want_pred": pred_b, k + "want_rec": rec_b,
                    k + "want_level": level_b, k + "want_abs_sum": abs_sum, k + "want_dist": dist})
        print("bit depth %d: %d PUs, %d items, abs_sum == 0 in %d" % (bd, n, int((abs_sum != icc.U32_MAX).sum()), int((abs_sum == 0).sum())))
    kit.save_golden(os.path.join(HERE, "intra_chroma_code.npz"), out)


if __name__ == "__main__":
    main()
