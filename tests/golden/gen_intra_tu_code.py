"""Generates tests/golden/intra_tu_code.npz: items of the intra RD loop's pixel pass (IntraSearch::xIntraCodingTUBlock, IntraSearch.cpp:1147-1316) whose every
stored value comes from the COMPILED REFERENCE's own functions, through the wrappers oracle/_ref/libvtmref.so exports: vtmref_intra_pred (predIntraAng with
xFilterReferenceSamples in front) and, as the chain steps of tests/rd_pass_kit.py call them, vtmref_pelop_area (AreaBuf::subtract), vtmref_tr_fwd_batch (xTrMxN_EMT), vtmref_quant_batch (Quant::quant),
vtmref_dequant_tr_inv_batch (Quant::dequant + xITrMxN_EMT), vtmref_pelop (PelBufferOps reco) and vtmref_dist (RdCost::xGetSSE).  Build machine only (needs
oracle/_ref/libvtmref.so, i.e. a build() where the reference exists):
    python tests/golden/gen_intra_tu_code.py

The tests' restatement (tests/intra_tu_code_cases.py) goes through the CPU restatement's steps; the generator asserts that it reproduces every stored value.
Nothing of the reference is copied; only the data is stored.  Inputs of the cases, not results of the reference: the modes, the filter decisions of the
explicit items, the transform pairs and quantiser parameters, and the packed references (gathered by orc_intra_fill_refs, which tests/golden/intra_fill.npz
checks against the reference's own calls)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

import intra_mode_cand_cases as imc  # noqa: E402
import intra_tu_code_cases as itc  # noqa: E402
import rd_pass_kit as kit  # noqa: E402
from oraclelib import p  # noqa: E402

# the reference pairs DCT-II only with DCT-II (g_aiTrSubsetInter holds DCT-VIII and DST-VII)
# (w, h, mode, filter_refs (None: the luma rule), tr_hor, tr_ver, qp - 6 (bd - 8), intra_slice, sign_hiding); mode -1: a given prediction
ROWS = [(4, 4, 0, None, 0, 0, 27, 1, 1), (4, 4, 34, 0, 2, 2, 22, 1, 0), (8, 8, 1, None, 0, 0, 32, 0, 1), (8, 8, 50, 1, 1, 2, 22, 1, 1),
        (16, 16, 2, None, 0, 0, 27, 1, 1), (16, 16, 18, 0, 2, 1, 32, 0, 0), (16, 16, 33, None, 1, 1, 22, 1, 1), (32, 32, 66, None, 0, 0, 27, 1, 1),
        (32, 32, 21, 1, 2, 2, 37, 0, 1), (64, 64, 0, None, 0, 0, 32, 1, 1), (64, 64, 45, 0, 0, 0, 22, 1, 0), (4, 8, 65, None, 0, 0, 27, 1, 1),
        (8, 4, 3, None, 2, 1, 22, 0, 1), (4, 16, 63, None, 1, 2, 27, 1, 0), (16, 4, 5, None, 0, 0, 32, 1, 1), (4, 32, 57, 1, 2, 2, 22, 1, 1),
        (32, 4, 7, None, 0, 0, 27, 0, 1), (4, 64, 61, None, 0, 0, 22, 1, 1), (64, 4, 9, None, 0, 0, 27, 1, 0), (8, 16, 34, None, 0, 0, 22, 1, 1),
        (16, 8, 2, 0, 1, 1, 32, 0, 1), (8, 32, 11, None, 2, 1, 27, 1, 1), (32, 8, 4, None, 0, 0, 22, 1, 0), (8, 64, 59, None, 0, 0, 32, 1, 1),
        (64, 8, 18, 1, 0, 0, 22, 0, 1), (16, 32, 50, None, 0, 0, 27, 1, 1), (32, 16, 29, 0, 2, 2, 22, 1, 1), (16, 64, 66, None, 0, 0, 32, 1, 0),
        (64, 16, 1, None, 0, 0, 27, 0, 1), (32, 64, 13, None, 0, 0, 22, 1, 1), (64, 32, 6, None, 0, 0, 63, 1, 1), (16, 16, -1, 0, 0, 0, 27, 1, 1),
        (8, 8, -1, 0, 2, 2, 22, 0, 1)]


def ref_item(R, tc, i, clp):
    """one item through the compiled reference -> (pred, levels, abs_sum, rec, dist)"""
    it = tc.items[i]
    u = tc.base.pus[int(it["pu"])]
    w, h, bd, mode = int(it["w"]), int(it["h"]), tc.bd, int(it["mode"])
    org = np.ascontiguousarray(tc.base.org[int(u["y"]):int(u["y"]) + h, int(u["x"]):int(u["x"]) + w])
    if mode == itc.PRED_GIVEN:
        pred = itc.block(tc.pred0, int(it["pred_off"]), int(it["pred_stride"]), w, h).copy()
    else:
        pred = np.zeros((h, w), np.int16)
        assert R.vtmref_intra_pred(p(tc.refs_of(int(it["pu"]))), p(pred), w, w, h, mode, clp[0], clp[1], bd, int(it["filt"]), None) == 0
    level, abs_sum, resi2 = kit.code_resi(kit.subtract(org, pred, bd, R), bd, int(it["tr_hor"]), int(it["tr_ver"]), int(it["qp"]), int(it["intra"]), int(it["sbh"]), R)
    rec = kit.reconstruct(pred, resi2, clp, bd, R)
    return pred, level, abs_sum, rec, kit.sse(org, rec, bd, R)


def main():
    R = kit.reference()
    out = {}
    for bd in (8, 10):
        rng = np.random.default_rng(8600 + bd)
        clp = (0, (1 << bd) - 1)
        base = itc.fresh_base(rng, bd, [(r[0], r[1]) for r in ROWS])
        specs = []
        for q, (w, h, mode, filt, th, tv, qp, intra, sbh) in enumerate(ROWS):
            f = int(imc.use_filtered(w, h, mode)) if filt is None and mode >= 0 else int(filt or 0)
            specs.append(dict(pu=q, mode=mode, filt=f, tr_hor=th, tr_ver=tv, qp=qp + 6 * (bd - 8), intra=intra, sbh=sbh))
        tc = itc.make(base, specs, rng)
        flags = itc.WRITE_PRED
        want = itc.restate(tc, flags)
        assert {int(v) for v in tc.items["filt"][tc.items["mode"] >= 0]} == {0, 1}
        pred_b, rec_b, level_b = tc.initial()
        n = len(tc.items)
        abs_sum, num_sig, dist = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint64)
        for i, it in enumerate(tc.items):
            w, h = int(it["w"]), int(it["h"])
            pred, level, abs_sum[i], rec, dist[i] = ref_item(R, tc, i, clp)
            num_sig[i] = np.count_nonzero(level)
            itc.block(pred_b, int(it["pred_off"]), int(it["pred_stride"]), w, h)[:] = pred
            itc.block(rec_b, int(it["rec_off"]), int(it["rec_stride"]), w, h)[:] = rec
            level_b[int(it["level_off"]):int(it["level_off"]) + w * h] = level
        kit.check_restatement(want, dict(pred=pred_b, rec=rec_b, level=level_b, abs_sum=abs_sum, num_sig=num_sig, dist=dist), bd)
        itc.check_conditions(tc, want)
        k = "bd%d_" % bd
        out.update({k + "rec": base.rec, k + "org": base.org, k + "pus": base.pus.view(np.uint8), k + "avail": base.avail, k + "items": tc.items.view(np.uint8),
                    k + "pred0": tc.pred0, k + "rec_size": np.int64(tc.rec_size), k + "level_size": np.int64(tc.level_size), k + "flags": np.int32(flags),
                    k + "want_pred": pred_b, k + "want_rec": rec_b, k + "want_level": level_b, k + "want_abs_sum": abs_sum, k + "want_num_sig": num_sig,
                    k + "want_dist": dist})
        print("bit depth %d: %d items, num_sig %s" % (bd, n, [int(v) for v in num_sig]))
    kit.save_golden(os.path.join(HERE, "intra_tu_code.npz"), out)


if __name__ == "__main__":
    main()
