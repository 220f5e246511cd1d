"""The device harness of vvcgpu_intra_luma_choose_batch and vvcgpu_intra_chroma_choose_batch (tests/test_gpu_intra_choose.py,
tools/intra_choose_time.py): one call of each entry through ops on uploaded arrays with canary-filled destinations, and the whole intra chain of a
list of CUs on one stream -- vvcgpu_intra_mode_cand_batch -> vvcgpu_intra_tu_code_batch / _dq_batch (FROM_LIST) -> vvcgpu_resi_rate_batch -> the luma
compare and commit -> vvcgpu_intra_chroma_code_batch / _dq_batch reading the committed plane -> vvcgpu_resi_rate_batch x 2 -> the chroma compare and
commit -- with what the restatement needs downloaded at the end."""
import numpy as np
import torch

import intra_choose_cases as icc
import intra_chroma_code_cases as icq
import intra_chroma_dq_cases as cdq
import intra_mode_cand_cases as imc
import intra_mode_cand_chain
import intra_tu_code_cases as itc
import intra_tu_dq_cases as tdq
import resi_rate_cases as rrc
from rd_pass_kit import LEVEL_CANARY, REC_CANARY, dev
from resi_rate_chain import Model, signed
from vvcsoftware_vtm_amd import abi, ops

CTX_CANARY = 0xEE


def canary_cost(shape):
    return torch.from_numpy(np.full(shape, icc.COST_CANARY, np.uint64).view(np.float64)).cuda()


def luma_inputs(c, tus):
    """the device arrays of a luma case: (pus, tus, abs_sum, num_sig, dist, mode_out, frac_bits)"""
    return (ops.struct_to_device(c["pus"]), ops.struct_to_device(tus)) + tuple(dev(signed(c[k])) for k in ("abs_sum", "num_sig", "dist", "mode_out", "frac_bits"))


def run_luma(c, tus, rec, level, ctx_out, rec_dst0, level_dst0, ctx_best0):
    """the entry on uploads of host arrays -> dict(cand_cost uint64, result, rec_dst, level_dst, ctx_best) on the host"""
    n_pu, n = len(c["pus"]), len(c["abs_sum"])
    pus, tus_d, abs_sum, num_sig, dist, mode_out, frac = luma_inputs(c, tus)
    rec_dst, level_dst = dev(rec_dst0), dev(level_dst0)
    ctx_best = None if ctx_best0 is None else dev(ctx_best0)
    cost, result = ops.intra_luma_choose_batch(pus, n_pu, tus_d, n, abs_sum, num_sig, dist, mode_out, frac, c["scale"], dev(rec), dev(level), rec_dst, level_dst,
                                               None if ctx_out is None else dev(ctx_out), ctx_best, canary_cost(n))
    torch.cuda.synchronize()
    return dict(cand_cost=cost.cpu().numpy().view(np.uint64), result=result.cpu().numpy().view(abi.INTRA_CHOOSE_RESULT), rec_dst=rec_dst.cpu().numpy(),
                level_dst=level_dst.cpu().numpy(), ctx_best=None if ctx_best is None else ctx_best.cpu().numpy())


def want_luma(c, tus, rec, level, ctx_out, rec_dst0, level_dst0, ctx_best0):
    """the restatement of the same call"""
    want = icc.luma_choose(c)
    want["rec_dst"], want["level_dst"], want["ctx_best"] = icc.luma_commit(c, want["result"], tus, rec, level, ctx_out, rec_dst0, level_dst0, ctx_best0)
    return want


def run_chroma(c, cand_rec, level, ctx_out, rec_dst0, level_dst0, ctx_best0):
    n = len(c["pus"])
    rec_dst, level_dst = dev(rec_dst0), dev(level_dst0)
    ctx_best = None if ctx_best0 is None else dev(ctx_best0)
    slot_cost = canary_cost((n, 6))
    _, result = ops.intra_chroma_choose_batch(ops.struct_to_device(c["cpus"]), ops.struct_to_device(c["pus"]), n, dev(signed(c["abs_sum"])),
                                              dev(signed(c["dist"])), dev(signed(c["frac_cb"])), dev(signed(c["frac_cr"])), c["scale"], dev(cand_rec), dev(level),
                                              rec_dst, level_dst, None if ctx_out is None else dev(ctx_out), ctx_best, slot_cost)
    torch.cuda.synchronize()
    return dict(slot_cost=slot_cost.cpu().numpy().view(np.uint64), result=result.cpu().numpy().view(abi.INTRA_CHROMA_CHOOSE_RESULT),
                rec_dst=rec_dst.cpu().numpy(), level_dst=level_dst.cpu().numpy(), ctx_best=None if ctx_best is None else ctx_best.cpu().numpy())


def want_chroma(c, cand_rec, level, ctx_out, rec_dst0, level_dst0, ctx_best0):
    want = icc.chroma_choose(c)
    want["rec_dst"], want["level_dst"], want["ctx_best"] = icc.chroma_commit(c, want["result"], cand_rec, level, ctx_out, rec_dst0, level_dst0, ctx_best0)
    return want


LUMA_KEYS = ("cand_cost", "result", "rec_dst", "level_dst", "ctx_best")
CHROMA_KEYS = ("slot_cost", "result", "rec_dst", "level_dst", "ctx_best")


def commit_buffers(c, rng, luma, n_rows):
    """candidate-side random context rows and canary-filled destinations for a case whose destinations are placed here
    -> (ctx_out, rec_dst0, level_dst0, ctx_best0)"""
    plane, store = (icc.place_luma_dst if luma else icc.place_chroma_dst)(c, rng)
    n = len(c["pus"])
    return (rng.integers(0, 128, (n_rows, abi.RESI_RATE_CTX_BYTES)).astype(np.uint8), np.full(plane, REC_CANARY, np.int16), np.full(store, LEVEL_CANARY, np.int32),
            np.full((n, abi.RESI_RATE_CTX_BYTES), CTX_CANARY, np.uint8))


# ---- the whole chain ---------------------------------------------------------------------------------------------------------------------------------
N_MODES, N_TR = 6, 2                                                        # slots asked of every list (the last ones lie beyond it), DCT-II and one EMT pair


def chain_case(dq, bd=10):
    """ten CUs, five of 8x8 and five of 16x16, in the planes of intra_mode_cand_cases; their chroma PUs (4x4, 8x8) with an LM slot, the luma block of
    each being the CU's block in the luma reconstruction plane -> a dict of host-side cases and records"""
    rng = np.random.default_rng(9500 + dq)
    rec, org = imc.fresh_planes(rng, bd)
    blocks = [(12 + 36 * (i % 5), 12 + 44 * (i // 5), 8 if i < 5 else 16, 8 if i < 5 else 16) for i in range(10)]
    base = itc.plain_case(bd, rec, org, blocks)
    for u in base.pus:
        u["bits"] = imc.random_bits(rng)
        u["mpm"] = [int(v) for v in rng.choice(imc.N_MODES, 3, replace=False)]
    specs = []
    for q, (x, y, w, h) in enumerate(blocks):
        pairs = itc.emt_pairs(w, h)
        for m in range(N_MODES):
            for t in range(N_TR):
                th, tv = pairs[0] if t == 0 else pairs[1 + (q + m) % 4]
                specs.append(dict(pu=q, mode=itc.FROM_LIST, row=q, slot=m, tr_hor=th, tr_ver=tv, qp=(27, 32, 37)[q % 3] + 6 * (bd - 8), intra=1, sbh=0 if dq else q % 2))
    luma = tdq.make(base, specs, rng) if dq else itc.make(base, specs, rng)
    tc = luma.tc if dq else luma
    n = len(tc.items)
    ritems = np.zeros(n, abi.RESI_RATE_ITEM)
    ritems["level_off"], ritems["w"], ritems["h"], ritems["luma"], ritems["dep_quant"] = tc.items["level_off"], tc.items["w"], tc.items["h"], 1, dq
    ritems["sign_hiding"], ritems["ts_flag"], ritems["emt_idx"], ritems["emt_thr"] = (0 if dq else tc.items["sbh"]), -1, np.arange(n) % N_TR, 1
    pus = np.zeros(len(blocks), abi.INTRA_CHOOSE_PU)
    for q, (x, y, w, h) in enumerate(blocks):
        u = pus[q]
        u["cand_first"], u["n_modes"], u["n_tr"], u["mpm"], u["mode_bits"] = q * N_MODES * N_TR, N_MODES, N_TR, base.pus[q]["mpm"], base.pus[q]["bits"]
        u["flags"] = abi.INTRA_CHOOSE_EMT_FLAG | (abi.INTRA_CHOOSE_FAST_EMT if q % 2 else 0)
        u["cbf_bits"], u["emt_cu_bits"] = rng.integers(1 << 10, 1 << 17, 2), int(rng.integers(1 << 10, 1 << 17))
        u["rec_dst_off"], u["rec_dst_stride"], u["level_dst_off"] = y * base.W + x, base.W, 4 + 260 * q
    # the chroma PUs: at half the CU's position; their luma block lies in the luma plane above, which the luma commit writes
    _, crec, corg = icq.planes(rng, bd)
    cspecs = [dict(w=w // 2, h=h // 2, pos=(x // 2, y // 2), modes=icq.cand_modes((2, 34, 50, 18, 66)[q % 5]), qp=30 + 6 * (bd - 8) + q % 4, sbh=0 if dq else q % 2)
              for q, (x, y, w, h) in enumerate(blocks)]
    pl = (np.zeros((2 * icq.CH, 2 * icq.CW), np.int16), crec, corg)
    chroma = cdq.make(rng, bd, cspecs, pl=pl) if dq else icq.make(rng, bd, cspecs, pl)
    cc = chroma.cc if dq else chroma
    for q, (x, y, w, h) in enumerate(blocks):                                # (make keeps the order: the list is grouped by shape already)
        assert (int(cc.pus[q]["w"]), int(cc.pus[q]["h"])) == (w // 2, h // 2)
        cc.pus[q]["luma_off"], cc.pus[q]["luma_stride"] = y * base.W + x, base.W
    cpus = np.zeros(len(blocks), abi.INTRA_CHROMA_CHOOSE_PU)
    for q, (x, y, w, h) in enumerate(blocks):
        u = cpus[q]
        u["mode_bits"], u["cbf_cb_bits"], u["cbf_cr_bits"] = rng.integers(1 << 13, 1 << 17, 6), rng.integers(1 << 10, 1 << 17, 2), rng.integers(1 << 10, 1 << 17, 4)
        u["dist_weight"] = rng.uniform(0.7, 1.6, 2)
        for comp in range(2):
            u["rec_dst_off"][comp], u["level_dst_off"][comp] = comp * icq.CW * icq.CH + (y // 2) * icq.CW + x // 2, 4 + 68 * (2 * q + comp)
        u["rec_dst_stride"] = icq.CW
    g = rrc.golden()
    ctx = np.stack([g["ctx_before"][2], g["ctx_before"][len(g["ctx_before"]) - 2]])      # a luma and a chroma row of the golden snapshots
    items_cb, items_cr = icc.chroma_rate_items(cc.pus, dq, ctx_idx=1)
    return dict(dq=dq, bd=bd, base=base, luma=luma, tc=tc, ritems=ritems, pus=pus, chroma=chroma, cc=cc, cpus=cpus, items_cb=items_cb, items_cr=items_cr,
                ctx=ctx, scale=float(rng.uniform(40.0, 300.0)), cscale=float(rng.uniform(40.0, 300.0)), est=g["est_bits"], nxt=g["next_state"])


def run_chain(k):
    """every call of the chain queued on the current stream, one synchronisation behind the last -> (the downloaded arrays, by name; the device
    tensors a second chroma call needs)"""
    bd, dq, tc, cc = k["bd"], k["dq"], k["tc"], k["cc"]
    clp = (0, (1 << bd) - 1)
    up = ops.struct_to_device
    # uploads first: nothing below waits for the host
    M = intra_mode_cand_chain.Device(k["base"])
    refs = M.fresh_refs()
    d, t = tc.descs()
    preds, tus = up(d), up(t)
    pred, rec, level = (dev(b) for b in tc.initial())
    model = Model(k["est"], k["nxt"])
    ctx = dev(k["ctx"])
    n, n_pu = len(tc.items), len(k["pus"])
    ritems, pus, cpus, cpu_pus = up(k["ritems"]), up(k["pus"]), up(k["cpus"]), up(cc.pus)
    ctx_out = torch.full((n, abi.RESI_RATE_CTX_BYTES), CTX_CANARY, dtype=torch.uint8, device="cuda")
    ctx_best = torch.full((n_pu, abi.RESI_RATE_CTX_BYTES), CTX_CANARY, dtype=torch.uint8, device="cuda")
    level_dst = torch.full((4 + 260 * n_pu + 8,), LEVEL_CANARY, dtype=torch.int32, device="cuda")
    cost = canary_cost(n)
    crefs0, cpred0, crec0, clevel0 = cc.initial()
    crefs, cpred, ccand, clevel = dev(crefs0), dev(cpred0), dev(crec0), dev(clevel0)
    fill = (dev(cc.rec.reshape(-1)), dev(cc.avail), up(cc.fill))
    corg = dev(cc.org.reshape(-1))
    items_cb, items_cr = up(k["items_cb"]), up(k["items_cr"])
    ctx_cb = torch.full((12 * n_pu, abi.RESI_RATE_CTX_BYTES), CTX_CANARY, dtype=torch.uint8, device="cuda")
    ctx_cr = torch.full_like(ctx_cb, CTX_CANARY)
    cctx_best = torch.full_like(ctx_best, CTX_CANARY)
    crec_dst = dev(cc.rec.reshape(-1).copy())
    clevel_dst = torch.full((4 + 68 * 2 * n_pu + 8,), LEVEL_CANARY, dtype=torch.int32, device="cuda")
    slot_cost = canary_cost((n_pu, 6))
    if dq:
        ldq, lrates = up(k["luma"].dq), up(k["luma"].rates)
        lws = ops.intra_tu_code_dq_workspace(tc.level_size, n)
        qdq, crates = up(k["chroma"].dq), up(k["chroma"].rates)
        cws = ops.intra_chroma_code_dq_workspace(cc.level_size, n_pu)
    torch.cuda.synchronize()
    # ---- the chain
    _, lists, _ = intra_mode_cand_chain.run_entry(M, imc.USE_MPM, 23.75, refs)
    if dq:
        out = ops.intra_tu_code_dq_batch(refs, preds, M.org, pred, rec, level, tus, ldq, n, lrates, len(k["luma"].rates), lists, 0, bd, clp, lws)
    else:
        out = ops.intra_tu_code_batch(refs, preds, M.org, pred, rec, level, tus, n, lists, 0, bd, clp)
    abs_sum, num_sig, dist, mode_out = out
    frac, _ = ops.resi_rate_batch(level, ritems, n, ctx, model.est, model.nxt, abs_sum, ctx_out)
    _, result = ops.intra_luma_choose_batch(pus, n_pu, tus, n, abs_sum, num_sig, dist, mode_out, frac, k["scale"], rec, level, M.rec, level_dst, ctx_out, ctx_best, cost)
    if dq:
        cabs, cdist = ops.intra_chroma_code_dq_batch(corg, cpu_pus, qdq, n_pu, cc.runs, crates, len(k["chroma"].rates), ccand, clevel, crefs, fill, M.rec, cpred, 0, bd,
                                                     clp, cws)
    else:
        cabs, cdist = ops.intra_chroma_code_batch(corg, cpu_pus, n_pu, cc.runs, ccand, clevel, crefs, fill, M.rec, cpred, 0, bd, clp)
    gate = cabs.reshape(-1)
    frac_cb, _ = ops.resi_rate_batch(clevel, items_cb, 12 * n_pu, ctx, model.est, model.nxt, gate, ctx_cb)
    frac_cr, _ = ops.resi_rate_batch(clevel, items_cr, 12 * n_pu, ctx_cb, model.est, model.nxt, gate, ctx_cr)
    _, cresult = ops.intra_chroma_choose_batch(cpus, cpu_pus, n_pu, cabs, cdist, frac_cb, frac_cr, k["cscale"], ccand, clevel, crec_dst, clevel_dst, ctx_cr, cctx_best,
                                               slot_cost)
    torch.cuda.synchronize()
    host = lambda x, view=None: x.cpu().numpy() if view is None else x.cpu().numpy().view(view)
    got = dict(lists=host(lists), abs_sum=host(abs_sum, np.uint32), num_sig=host(num_sig, np.uint32), dist=host(dist, np.uint64), mode_out=host(mode_out),
               frac=host(frac, np.uint64), rec=host(rec), level=host(level), ctx_out=host(ctx_out), cand_cost=host(cost, np.uint64),
               result=host(result, abi.INTRA_CHOOSE_RESULT), plane=host(M.rec), level_dst=host(level_dst), ctx_best=host(ctx_best),
               cabs=host(cabs, np.uint32), cdist=host(cdist, np.uint64), ccand=host(ccand), clevel=host(clevel), frac_cb=host(frac_cb, np.uint64),
               frac_cr=host(frac_cr, np.uint64), ctx_cb=host(ctx_cb), ctx_cr=host(ctx_cr), slot_cost=host(slot_cost, np.uint64),
               cresult=host(cresult, abi.INTRA_CHROMA_CHOOSE_RESULT), crec_dst=host(crec_dst), clevel_dst=host(clevel_dst), cctx_best=host(cctx_best))
    return got


def chroma_pass_alone(k, plane):
    """the chroma pass of the chain's case by itself with luma_base = an upload of `plane` -> (abs_sum, dist) on the host"""
    bd, dq, cc = k["bd"], k["dq"], k["cc"]
    clp = (0, (1 << bd) - 1)
    up = ops.struct_to_device
    crefs0, cpred0, crec0, clevel0 = cc.initial()
    fill = (dev(cc.rec.reshape(-1)), dev(cc.avail), up(cc.fill))
    args = (dev(crec0), dev(clevel0), dev(crefs0), fill, dev(plane), dev(cpred0), 0, bd, clp)
    if dq:
        a, d = ops.intra_chroma_code_dq_batch(dev(cc.org.reshape(-1)), up(cc.pus), up(k["chroma"].dq), len(cc.pus), cc.runs, up(k["chroma"].rates),
                                              len(k["chroma"].rates), *args)
    else:
        a, d = ops.intra_chroma_code_batch(dev(cc.org.reshape(-1)), up(cc.pus), len(cc.pus), cc.runs, *args)
    torch.cuda.synchronize()
    return a.cpu().numpy().view(np.uint32), d.cpu().numpy().view(np.uint64)
