"""Generates tests/golden/ts_dq.npz: small lists for vvcgpu_inter_resi_code_dq_batch under VVCGPU_INTER_RESI_DQ_TS and vvcgpu_intra_tu_code_dq_batch under
VVCGPU_INTRA_TU_DQ_TS whose every stored result comes from the COMPILED REFERENCE's own functions, through the wrappers oracle/_ref/libvtmref.so exports, as
the chain steps of tests/rd_pass_kit.py call them.  The transform-skip candidate of a 4x4 block is the COMPOSITION of three of them -- vtmref_tr_fwd_batch with
tr_hor = 3 (TrQuant::xTransformSkip), vtmref_depquant (DQIntern::DepQuant::quant), vtmref_dequant_tr_inv_batch with tr_hor = 3 and dep_quant = 1
(DQIntern::Quantizer::dequantBlock + TrQuant::xITransformSkip) -- as TrQuant::transformNxN / invTransformNxN compose them; oracle/ has no wrapper around
transformNxN with tu.transformSkip set (docs/ORACLE.md says why the composition is the same thing).  Build machine only (needs oracle/_ref/libvtmref.so):
    python tests/golden/gen_ts_dq.py

The tests' restatement (tests/ts_dq_cases.py) goes through the CPU restatement's steps; the generator asserts that it reproduces every stored value.
Nothing of the reference is copied; only the data is stored.  Inputs of the cases, not results of the reference: the planes, the predictions, the
transform candidates, the QPs, the lambdas and the (ctxQp, initId) pairs the rate tables are derived for."""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

import inter_resi_code_cases as irc  # noqa: E402
import inter_resi_dq_cases as dqc  # noqa: E402
import intra_mode_cand_cases as imc  # noqa: E402
import intra_tu_code_cases as itc  # noqa: E402
import intra_tu_dq_cases as tdq  # noqa: E402
import rd_pass_kit as kit  # noqa: E402
import ts_dq_cases as ts  # noqa: E402
from oraclelib import p  # noqa: E402

ROWS_H = 40                                                                  # rows of the planes the file stores with content


def ref_slot(R, resi, bd, code, qp, lam, ctx):
    """one slot of a contiguous residual through the compiled reference -> (levels [w h], abs_sum, resi', its rate table); code TS: the skip candidate"""
    h, w = resi.shape
    rt = np.zeros(1, dqc.RATES)
    if code == ts.TS:
        level, abs_sum, resi2 = ts.code_ts(resi, bd, qp, lam, None, rt, R, ctx)
        return level.reshape(-1), abs_sum, resi2, rt
    th, tv = code % 3, code // 3
    coef, level = kit.forward(resi, bd, th, tv, R), np.zeros(w * h, np.int32)
    abs_sum = int(R.vtmref_depquant(p(coef), p(level), w, h, ctx[0], bd, qp, C.c_double(lam), ctx[1], ctx[2], p(rt)))
    return level, abs_sum, kit.dequant_inverse(level, w, h, bd, th, tv, qp, 1, R), rt


def inter_rows():
    """(w, h, slots, comp): 4x4 blocks with the skip slot alone, behind DCT-II and behind an EMT pair, luma and Cb; other shapes beside them"""
    out = []
    for j in range(12):
        out.append((4, 4, ([0, ts.TS], [ts.TS], [0, 4, ts.TS])[j % 3], j % 2))
    return out + [(8, 8, [0, 4], 0), (4, 16, [0], 1), (16, 4, [0, 8], 0), (32, 32, [0], 0)]


def gen_inter(R, bd, out):
    rng = np.random.default_rng(9700 + bd)
    clp = (0, (1 << bd) - 1)
    plane = np.ascontiguousarray(irc.fresh_plane(rng, bd)[:ROWS_H])
    specs, ctx = [], []
    for j, (w, h, tr, comp) in enumerate(inter_rows()):
        x, _ = irc.place(rng, w, h, band=j % 3)
        y = int(rng.integers(0, ROWS_H - h + 1))
        specs.append(dict(x=x, y=y, w=w, h=h, tr=tr, qp=ts.QPS[j % 3] + 6 * (bd - 8), luma=1 - comp, rates_idx=j,
                          pred=ts.amp_pred(rng, plane[y:y + h, x:x + w], bd, ts.AMPS[(j // 3) % 3])))
        ctx.append((comp, int(rng.integers(20, 45)), int(rng.integers(0, 3))))
    n = len(specs)
    case = dqc.make(bd, plane, specs, rng, rates=np.zeros(n, dqc.RATES))
    flags = ts.DQ_TS | ts.WRITE_REC
    resi_b, rec_b, level_b = case.initial()
    abs_sum = np.full((n, ts.SLOTS), ts.U32_MAX, np.uint32)
    dist_resi, dist_rec = np.full((n, ts.SLOTS), ts.U64_MAX, np.uint64), np.full((n, ts.SLOTS), ts.U64_MAX, np.uint64)
    zero_dist = np.zeros(n, np.uint64)
    for i, it in enumerate(case.items):
        w, h, sz = int(it["w"]), int(it["h"]), int(it["w"]) * int(it["h"])
        org = np.ascontiguousarray(irc.block(case.org, int(it["org_off"]), int(it["org_stride"]), w, h))
        pred = np.ascontiguousarray(irc.block(case.pred, int(it["pred_off"]), int(it["pred_stride"]), w, h))
        resi = kit.subtract(org, pred, bd, R)
        zero_dist[i] = kit.sse(np.zeros((h, w), np.int16), resi, bd, R)
        table = None
        for k in range(ts.SLOTS):
            code = int(it["tr"][k])
            if code < 0:
                continue
            level, asum, resi2, rt = ref_slot(R, resi, bd, code, int(it["qp"]), float(case.dq[i]["lambda"]), ctx[i])
            assert table is None or table.tobytes() == rt.tobytes()          # one table per (shape, component, context state): the skip slot's is the others'
            table = rt
            rec = kit.reconstruct(pred, resi2, clp, bd, R)
            co, lo = int(it["cand_off"]) + k * sz, int(it["level_off"]) + k * sz
            resi_b[co:co + sz], rec_b[co:co + sz], level_b[lo:lo + sz] = resi2.reshape(-1), rec.reshape(-1), level
            abs_sum[i, k], dist_resi[i, k], dist_rec[i, k] = asum, kit.sse(resi, resi2, bd, R), kit.sse(org, rec, bd, R)
        case.rates[i] = table[0]
    want = ts.inter_restate(case, flags)
    kit.check_restatement(want, dict(resi=resi_b, rec=rec_b, level=level_b, abs_sum=abs_sum, dist_resi=dist_resi, dist_rec=dist_rec, zero_dist=zero_dist), bd)
    assert ((abs_sum != ts.U32_MAX) == (case.items["tr"] >= 0)).all()        # every slot of the file is a served one
    slots = ts.check_levels(case, want)
    k = "inter_bd%d_" % bd
    out.update({k + "org": case.org, k + "pred": case.pred, k + "items": case.items.view(np.uint8), k + "dq": case.dq.view(np.uint8),
                k + "rates": case.rates.view(np.int32), k + "cand_size": np.int64(case.cand_size), k + "level_size": np.int64(case.level_size),
                k + "flags": np.int32(flags), k + "want_resi": resi_b, k + "want_rec": rec_b, k + "want_level": level_b, k + "want_abs_sum": abs_sum,
                k + "want_dist_resi": dist_resi, k + "want_dist_rec": dist_rec, k + "want_zero_dist": zero_dist})
    print("inter, bit depth %d: %d items, %d skip slots, %d of them with a level" % (bd, n, slots, (ts.ts_served(case) & (abs_sum > 0)).sum()))


def gen_intra(R, bd, out):
    rng = np.random.default_rng(9750 + bd)
    clp = (0, (1 << bd) - 1)
    rec, org = imc.fresh_planes(rng, bd)
    rec[ROWS_H:], org[ROWS_H:] = 0, 0                                         # (the PUs and their references lie above: the file stays small)
    shapes = [(4, 4)] * 8 + [(8, 8), (16, 16)]
    blocks = [(8 + 20 * q, 8 + 4 * (q % 3), w, h) for q, (w, h) in enumerate(shapes)]
    base = itc.plain_case(bd, rec, org, blocks, rng)
    specs, ctx, givens = [], [], {}
    for q, (w, h) in enumerate(shapes):
        comp = q % 2 if w == 4 else 0
        c = (comp, int(rng.integers(20, 45)), int(rng.integers(0, 3)))
        mode = itc.PRED_GIVEN if q % 4 == 3 else itc.MODES[q % len(itc.MODES)]
        for t in range(2 if w == 4 else 1):
            if mode == itc.PRED_GIVEN:
                givens[len(specs)] = ts.given_for(np.random.default_rng(q), base, q, bd, ts.AMPS[q % 3])
            specs.append(dict(pu=q, mode=mode, filt=q % 2, tr_hor=ts.TSKIP * t, tr_ver=t * (q % 3), qp=ts.QPS[q % 3] + 6 * (bd - 8), luma=1 - comp,
                              lam=float(rng.uniform(5, 400)), rates_idx=len(specs)))
            ctx.append(c)
    n = len(specs)
    case = tdq.make(base, specs, rng, givens=givens, rates=np.zeros(n, tdq.RATES))
    tc = case.tc
    flags = ts.TU_DQ_TS | ts.WRITE_PRED
    pred_b, rec_b, level_b = tc.initial()
    abs_sum, num_sig, dist = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint64)
    for i, it in enumerate(tc.items):
        u = tc.base.pus[int(it["pu"])]
        w, h, mode = int(it["w"]), int(it["h"]), int(it["mode"])
        o = np.ascontiguousarray(tc.base.org[int(u["y"]):int(u["y"]) + h, int(u["x"]):int(u["x"]) + w])
        if mode == itc.PRED_GIVEN:
            pred = itc.block(tc.pred0, int(it["pred_off"]), int(it["pred_stride"]), w, h).copy()
        else:
            pred = np.zeros((h, w), np.int16)
            assert R.vtmref_intra_pred(p(tc.refs_of(int(it["pu"]))), p(pred), w, w, h, mode, clp[0], clp[1], bd, int(it["filt"]), None) == 0
        code = ts.TS if int(it["tr_hor"]) == ts.TSKIP else int(it["tr_hor"]) + 3 * int(it["tr_ver"])
        level, abs_sum[i], resi2, rt = ref_slot(R, kit.subtract(o, pred, bd, R), bd, code, int(it["qp"]), float(case.dq[i]["lambda"]), ctx[i])
        r = kit.reconstruct(pred, resi2, clp, bd, R)
        case.rates[i], num_sig[i], dist[i] = rt[0], np.count_nonzero(level), kit.sse(o, r, bd, R)
        itc.block(pred_b, int(it["pred_off"]), int(it["pred_stride"]), w, h)[:] = pred
        itc.block(rec_b, int(it["rec_off"]), int(it["rec_stride"]), w, h)[:] = r
        level_b[int(it["level_off"]):int(it["level_off"]) + w * h] = level
    want = ts.intra_restate(case, flags)
    kit.check_restatement(want, dict(pred=pred_b, rec=rec_b, level=level_b, abs_sum=abs_sum, num_sig=num_sig, dist=dist), bd)
    assert (want["abs_sum"] != ts.U32_MAX).all()                              # every item of the file is a served one
    skips = ts.check_tu_levels(case, want)
    k = "intra_bd%d_" % bd
    out.update({k + "rec": base.rec, k + "org": base.org, k + "pus": base.pus.view(np.uint8), k + "avail": base.avail, k + "items": tc.items.view(np.uint8),
                k + "dq": case.dq.view(np.uint8), k + "rates": case.rates.view(np.int32), k + "pred0": tc.pred0, k + "rec_size": np.int64(tc.rec_size),
                k + "level_size": np.int64(tc.level_size), k + "flags": np.int32(flags), k + "want_pred": pred_b, k + "want_rec": rec_b, k + "want_level": level_b,
                k + "want_abs_sum": abs_sum, k + "want_num_sig": num_sig, k + "want_dist": dist})
    print("intra, bit depth %d: %d items, %d skip items, %d of them with a level" % (bd, n, skips, (ts.tu_ts(tc) & (abs_sum > 0)).sum()))


def main():
    R = kit.reference()
    out = {}
    for bd in (8, 10):
        gen_inter(R, bd, out)
        gen_intra(R, bd, out)
    kit.save_golden(os.path.join(HERE, "ts_dq.npz"), out)


if __name__ == "__main__":
    main()
