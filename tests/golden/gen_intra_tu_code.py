"""Generates tests/golden/intra_tu_code.npz: items of the intra RD loop's pixel pass (IntraSearch::xIntraCodingTUBlock, IntraSearch.cpp:1147-1316) whose every
stored value comes from the COMPILED REFERENCE's own functions, through the wrappers oracle/_ref/libvtmref.so exports: vtmref_intra_pred (predIntraAng with
xFilterReferenceSamples in front), vtmref_pelop_area (AreaBuf::subtract), vtmref_tr_fwd_batch (xTrMxN_EMT), vtmref_quant_batch (Quant::quant),
vtmref_dequant_tr_inv_batch (Quant::dequant + xITrMxN_EMT), vtmref_pelop (PelBufferOps reco) and vtmref_dist (RdCost::xGetSSE).  Build machine only (needs
oracle/_ref/libvtmref.so, i.e. a build() where the reference exists):
    python tests/golden/gen_intra_tu_code.py

The tests' restatement (tests/intra_tu_code_cases.py) goes through the CPU restatement's steps; the generator asserts that it reproduces every stored value.
Nothing of the reference is copied; only the data is stored.  Inputs of the cases, not results of the reference: the modes, the filter decisions of the
explicit items, the transform pairs and quantiser parameters, and the packed references (gathered by orc_intra_fill_refs, which tests/golden/intra_fill.npz
checks against the reference's own calls)."""
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
from oraclelib import p, ref  # noqa: E402
from vvcsoftware_vtm_amd.abi import DQTR_DESC, QUANT_DESC, TR_DESC  # noqa: E402

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
    resi, resi2, rec = np.zeros((h, w), np.int16), np.zeros((h, w), np.int16), np.zeros((h, w), np.int16)
    coef, level, dqc = np.zeros(w * h, np.int32), np.zeros(w * h, np.int32), np.zeros(w * h, np.int32)
    abs_sum = np.zeros(1, np.uint32)
    tr = np.zeros(1, TR_DESC); tr[0] = (0, 0, w, w, h, it["tr_hor"], it["tr_ver"], 0, 0)
    qd = np.zeros(1, QUANT_DESC); qd[0] = (0, 0, w, h, it["intra"], it["sbh"], 0, it["qp"], 0)
    dq = np.zeros(1, DQTR_DESC); dq[0] = (0, 0, w, w, h, it["tr_hor"], it["tr_ver"], 0, 0, it["qp"])
    R.vtmref_pelop_area(3, p(org), w, p(pred), w, p(resi), w, w, h, 0, bd, clp[0], clp[1])
    assert R.vtmref_tr_fwd_batch(p(resi), p(coef), p(tr), 1, bd) == 0
    assert R.vtmref_quant_batch(p(coef), p(level), p(qd), 1, bd, p(abs_sum)) == 0
    assert R.vtmref_dequant_tr_inv_batch(p(level), p(resi2), p(dq), 1, bd, p(dqc)) == 0
    R.vtmref_pelop(1, 1, p(pred), w, p(resi2), w, p(rec), w, w, h, 0, 0, 0, 1, bd, clp[0], clp[1])
    dist = R.vtmref_dist(2, 1, p(org), w, p(rec), w, w, h, bd, 0)
    return pred, level, int(abs_sum[0]), rec, int(dist)


def main():
    R = ref()
    R.vtmref_dist.restype = C.c_uint64
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
        for k, v in (("pred", pred_b), ("rec", rec_b), ("level", level_b), ("abs_sum", abs_sum), ("num_sig", num_sig), ("dist", dist)):
            assert np.array_equal(want[k], v), (bd, k)                       # the restatement reproduces every stored value
        itc.check_conditions(tc, want)
        k = "bd%d_" % bd
        out.update({k + "rec": base.rec, k + "org": base.org, k + "pus": base.pus.view(np.uint8), k + "avail": base.avail, k + "items": tc.items.view(np.uint8),
                    k + "pred0": tc.pred0, k + "rec_size": np.int64(tc.rec_size), k + "level_size": np.int64(tc.level_size), k + "flags": np.int32(flags),
                    k + "want_pred": pred_b, k + "want_rec": rec_b, k + "want_level": level_b, k + "want_abs_sum": abs_sum, k + "want_num_sig": num_sig,
                    k + "want_dist": dist})
        print("bit depth %d: %d items, num_sig %s" % (bd, n, [int(v) for v in num_sig]))
    path = os.path.join(HERE, "intra_tu_code.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) <= 400 * 1024


if __name__ == "__main__":
    main()
