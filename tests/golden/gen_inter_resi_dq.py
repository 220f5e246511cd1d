"""Generates tests/golden/inter_resi_dq.npz: items of the inter residual pixel pass under DepQuant 1 (InterSearch::encodeResAndCalcRdInterCU with transformNxN /
invTransformNxN going through DQIntern::DepQuant) whose every stored result comes from the COMPILED REFERENCE's own functions, through the wrappers
oracle/_ref/libvtmref.so exports, as the chain steps of tests/rd_pass_kit.py call them: vtmref_pelop_area (AreaBuf::subtract), vtmref_tr_fwd_batch (xTrMxN_EMT), vtmref_depquant (DepQuant::quant; it hands back the
rate tables it derived from its CABAC contexts), vtmref_dequant_tr_inv_batch with dep_quant = 1 (DepQuant::dequant + xITrMxN_EMT), vtmref_pelop (PelBufferOps
reco) and vtmref_dist (RdCost::xGetSSE).  Build machine only (needs oracle/_ref/libvtmref.so, i.e. a build() where the reference exists):
    python tests/golden/gen_inter_resi_dq.py

The tests' restatement (tests/inter_resi_dq_cases.py) goes through the CPU restatement's steps; the generator asserts that it reproduces every stored value.
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
import rd_pass_kit as kit  # noqa: E402
from oraclelib import p  # noqa: E402

ROWS_H = 96                                                                  # rows of the original plane the file stores


def rows():
    """one row per item -> (w, h, slots, qp - 6 (bd - 8), comp): all 25 shapes with DCT-II; the four inter-EMT pairs on the squares 4 .. 32 and some
    rectangles; luma and Cb; QPs 22 .. 37, the largest QP"""
    out = []
    qps = (22, 27, 32, 37, 24, 29, 35)
    for k, (w, h) in enumerate(dqc.all_shapes()):
        tr = [0]
        if w == h and w <= 32:
            tr += list(dqc.EMT)
        elif w <= 32 and h <= 32 and k % 3 == 0:
            tr += [dqc.EMT[k % 4], dqc.EMT[(k + 1) % 4]]
        out.append((w, h, tr, qps[k % len(qps)], 1 if max(w, h) <= 32 and k % 2 else 0))
    out += [(16, 16, [0, 8], 63, 0), (8, 8, [0, 4], 63, 1), (4, 4, [0, 5], 63, 0), (64, 64, [0], 63, 0), (32, 32, [0, 7], 22, 1)]
    return out


def ref_item(R, case, i, clp, comp, cq, init):
    """one item through the compiled reference -> (zero_dist, its rate table, [(k, levels, abs_sum, resi', rec, dist_resi, dist_rec)])"""
    it, q = case.items[i], case.dq[i]
    w, h, bd = int(it["w"]), int(it["h"]), case.bd
    org = np.ascontiguousarray(irc.block(case.org, int(it["org_off"]), int(it["org_stride"]), w, h))
    pred = np.ascontiguousarray(irc.block(case.pred, int(it["pred_off"]), int(it["pred_stride"]), w, h))
    resi = kit.subtract(org, pred, bd, R)
    zero_dist = kit.sse(np.zeros((h, w), np.int16), resi, bd, R)
    slots, table = [], None
    for k in range(dqc.SLOTS):
        code = int(it["tr"][k])
        if code < 0:
            continue
        th, tv = code % 3, code // 3
        coef, level, rt = kit.forward(resi, bd, th, tv, R), np.zeros(w * h, np.int32), np.zeros(1, dqc.RATES)
        abs_sum = int(R.vtmref_depquant(p(coef), p(level), w, h, comp, bd, int(it["qp"]), C.c_double(float(q["lambda"])), cq, init, p(rt)))
        resi2 = kit.dequant_inverse(level, w, h, bd, th, tv, int(it["qp"]), 1, R)
        rec = kit.reconstruct(pred, resi2, clp, bd, R)
        assert table is None or table.tobytes() == rt.tobytes()              # one table per (shape, component, context state)
        table = rt
        slots.append((k, level, abs_sum, resi2, rec, kit.sse(resi, resi2, bd, R), kit.sse(org, rec, bd, R)))
    return zero_dist, table[0], slots


def main():
    R = kit.reference()
    out = {}
    for bd in (8, 10):
        rng = np.random.default_rng(8900 + bd)
        clp = (0, (1 << bd) - 1)
        plane = np.ascontiguousarray(irc.fresh_plane(rng, bd)[:ROWS_H])
        specs, ctx = [], []
        for q, (w, h, tr, qp, comp) in enumerate(rows()):
            x, _ = irc.place(rng, w, h, band=q % 3)
            # lambda and the context state the rate tables are derived for: as gen_golden.py's gen_depquant
            specs.append(dict(x=x, y=int(rng.integers(0, ROWS_H - h + 1)), w=w, h=h, tr=tr, qp=qp + 6 * (bd - 8), luma=1 - comp, lam=float(rng.uniform(5, 400)), rates_idx=q))
            ctx.append((comp, int(rng.integers(20, 45)), int(rng.integers(0, 3))))
        n = len(specs)
        case = dqc.make(bd, plane, specs, rng, rates=np.zeros(n, dqc.RATES))
        flags = dqc.WRITE_REC
        resi_b, rec_b, level_b = case.initial()
        abs_sum = np.full((n, dqc.SLOTS), dqc.U32_MAX, np.uint32)
        dist_resi, dist_rec = np.full((n, dqc.SLOTS), dqc.U64_MAX, np.uint64), np.full((n, dqc.SLOTS), dqc.U64_MAX, np.uint64)
        zero_dist = np.zeros(n, np.uint64)
        for i, it in enumerate(case.items):
            sz = int(it["w"]) * int(it["h"])
            zero_dist[i], case.rates[i], slots = ref_item(R, case, i, clp, *ctx[i])
            for (k, level, asum, resi2, rec, dr, dc) in slots:
                co, lo = int(it["cand_off"]) + k * sz, int(it["level_off"]) + k * sz
                resi_b[co:co + sz], rec_b[co:co + sz], level_b[lo:lo + sz] = resi2.reshape(-1), rec.reshape(-1), level
                abs_sum[i, k], dist_resi[i, k], dist_rec[i, k] = asum, dr, dc
        want = dqc.restate(case, flags)
        served = abs_sum != dqc.U32_MAX
        assert served.sum() == sum(len(r[2]) for r in rows())                # every slot of the file is a served one
        kit.check_restatement(want, dict(resi=resi_b, rec=rec_b, level=level_b, abs_sum=abs_sum, dist_resi=dist_resi, dist_rec=dist_rec, zero_dist=zero_dist), bd)
        assert (served & (abs_sum > 0)).sum() * 3 >= served.sum()
        assert (served & (abs_sum == 0)).any()                               # the early return
        assert (served & (dist_rec != dist_resi)).any()                      # the clip bites
        assert len({case.rates[i].tobytes() for i in range(n)}) >= 4
        k = "bd%d_" % bd
        out.update({k + "org": case.org, k + "pred": case.pred, k + "items": case.items.view(np.uint8), k + "dq": case.dq.view(np.uint8),
                    k + "rates": case.rates.view(np.int32), k + "cand_size": np.int64(case.cand_size), k + "level_size": np.int64(case.level_size),
                    k + "flags": np.int32(flags), k + "want_resi": resi_b, k + "want_rec": rec_b, k + "want_level": level_b, k + "want_abs_sum": abs_sum,
                    k + "want_dist_resi": dist_resi, k + "want_dist_rec": dist_rec, k + "want_zero_dist": zero_dist})
        print("bit depth %d: %d items, %d slots, %d all-zero, the clip bites in %d, %d distinct rate tables" % (
            bd, n, served.sum(), (served & (abs_sum == 0)).sum(), (served & (dist_rec != dist_resi)).sum(), len({case.rates[i].tobytes() for i in range(n)})))
    kit.save_golden(os.path.join(HERE, "inter_resi_dq.npz"), out)


if __name__ == "__main__":
    main()
