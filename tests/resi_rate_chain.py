"""The device harness of vvcgpu_resi_rate_batch and vvcgpu_inter_resi_choose_batch (tests/test_gpu_resi_rate.py, tools/resi_rate_time.py): one call of
each entry through ops on uploaded arrays, and the three-call chain behind vvcgpu_inter_resi_code_batch / _dq_batch -- the rate items of the pixel pass'
level blocks, the inputs of the compare -- with its restatement over downloaded levels."""
import numpy as np
import torch

import resi_rate_cases as rrc
from rd_pass_kit import dev
from vvcsoftware_vtm_amd import abi, ops

CTX_CANARY = 0xEE                                                            # what ctx_out holds before a call


def signed(a):
    """an unsigned host array as torch holds it"""
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.itemsize]) if a.dtype.kind == "u" and a.itemsize > 1 else a


class Model:
    """the two model tables on the device, uploaded once"""
    def __init__(self, est, nxt):
        self.est, self.nxt = dev(signed(est)), dev(nxt)


def run_rate(M, level, items, ctx, gate=None):
    """the entry on uploads of host arrays -> dict(frac_bits, num_sig, ctx_out) on the host; ctx_out starts as CTX_CANARY"""
    n = len(items)
    out = torch.full((n, abi.RESI_RATE_CTX_BYTES), CTX_CANARY, dtype=torch.uint8, device="cuda")
    frac, nsig = ops.resi_rate_batch(dev(level), ops.struct_to_device(items), n, dev(ctx), M.est, M.nxt, None if gate is None else dev(signed(gate)), out)
    torch.cuda.synchronize()
    return dict(frac_bits=frac.cpu().numpy().view(np.uint64), num_sig=nsig.cpu().numpy().view(np.uint32), ctx_out=out.cpu().numpy())


def want_rate(level, items, gate, ctx, est, nxt):
    """the restatement over the same arrays, ctx_out starting as CTX_CANARY"""
    return rrc.restate(level, items, gate, ctx, est, nxt, np.full((len(items), abi.RESI_RATE_CTX_BYTES), CTX_CANARY, np.uint8))


CHOOSE_KEYS = ("slot", "cbf", "abs_sum_out", "dist", "bits", "min_cost")


def run_choose(c):
    """the compare on uploads of the arrays of rrc.random_choose -> the dict of rrc.choose"""
    n = len(c["tr"])
    items = np.zeros(n, abi.INTER_RESI_ITEM)
    items["tr"] = c["tr"]
    got = ops.inter_resi_choose_batch(ops.struct_to_device(items), n, dev(signed(c["abs_sum"])), dev(signed(c["dist_resi"])), dev(signed(c["zero_dist"])),
                                      dev(signed(c["frac_bits"])), dev(signed(c["cbf_bits"])), dev(c["prev"]), dev(c["weight"]), c["scale"])
    torch.cuda.synchronize()
    views = dict(abs_sum_out=np.uint32, dist=np.uint64, bits=np.uint64)
    return {k: (t.cpu().numpy().view(views[k]) if k in views else t.cpu().numpy()) for k, t in zip(CHOOSE_KEYS, got)}


def same_choose(got, want):
    for k in CHOOSE_KEYS:
        assert got[k].tobytes() == want[k].tobytes(), (k, np.flatnonzero(got[k] != want[k])[:8])


# ---- the chain behind the inter residual pixel pass ------------------------------------------------------------------------------------------------
def rate_items(inter_items, luma, dep_quant):
    """the rate items 6 i + k of the pixel pass' items: the levels of slot k, row 0 (luma) or 1 (chroma) of the contexts, the transform-skip flag on the
    blocks the pass tries transform skip on (no EMT slots), the EMT index on the luma blocks with EMT slots"""
    it, k = inter_items, np.arange(abi.INTER_RESI_SLOTS)[None]
    luma = np.asarray(luma) != 0
    codes = it["tr"].astype(np.int64)
    emt, has_ts = np.isin(codes, (4, 5, 7, 8)).any(1), (codes == abi.INTER_RESI_TS).any(1)
    out = np.zeros((len(it), abi.INTER_RESI_SLOTS), abi.RESI_RATE_ITEM)
    out["level_off"] = it["level_off"][:, None] + k * (it["w"].astype(np.int64) * it["h"])[:, None]
    out["ctx_idx"], out["w"], out["h"], out["luma"] = np.where(luma, 0, 1)[:, None], it["w"][:, None], it["h"][:, None], luma[:, None]
    out["dep_quant"], out["sign_hiding"] = dep_quant, 0 if dep_quant else it["sign_hiding"][:, None]
    out["ts_flag"] = np.where((emt | ~has_ts)[:, None], -1, codes == abi.INTER_RESI_TS)
    out["emt_idx"] = np.where((emt & luma)[:, None] & (k < 4) & (codes != abi.INTER_RESI_TS), k, -1)
    out["emt_inter"] = (emt & luma)[:, None]
    return out.reshape(-1)


def chain_inputs(n, seed):
    """the compare's inputs that do not come from the device: cbf bits, Cr items behind the item before them, chroma weights, the scale"""
    rng = np.random.default_rng(seed)
    cbf_bits = rng.integers(1 << 10, 1 << 17, (n, 4)).astype(np.uint64)
    prev = np.where((np.arange(n) % 3 == 2), np.arange(n) - 1, -1).astype(np.int32)
    weight = np.where(np.arange(n) % 3 == 0, 1.0, rng.uniform(0.7, 1.6, n))
    return cbf_bits, prev, weight, float(rng.uniform(30.0, 400.0))


def run_chain(D, M, ritems, ctx, cbf_bits, prev, weight, scale):
    """the pixel pass (D: its Device), the rate of its level blocks with gate = abs_sum, the compare: one stream, nothing downloaded in between
    -> (the level buffer, abs_sum, the rate outputs, the compare's outputs) on the host"""
    resi, rec, level = D.fresh()
    abs_sum, dist_resi, _, zero_dist = D.run_entry(resi, None, level)
    n6 = len(ritems)
    frac, nsig = ops.resi_rate_batch(level, ops.struct_to_device(ritems), n6, dev(ctx), M.est, M.nxt, abs_sum)
    got = ops.inter_resi_choose_batch(D.items_dev, D.n, abs_sum, dist_resi, zero_dist, frac, dev(signed(cbf_bits)), dev(prev), dev(weight), scale)
    torch.cuda.synchronize()
    views = dict(abs_sum_out=np.uint32, dist=np.uint64, bits=np.uint64)
    chosen = {k: (t.cpu().numpy().view(views[k]) if k in views else t.cpu().numpy()) for k, t in zip(CHOOSE_KEYS, got)}
    rate = dict(frac_bits=frac.cpu().numpy().view(np.uint64), num_sig=nsig.cpu().numpy().view(np.uint32))
    return (level.cpu().numpy(), abs_sum.cpu().numpy().view(np.uint32), dist_resi.cpu().numpy().view(np.uint64), zero_dist.cpu().numpy().view(np.uint64),
            rate, chosen)


def want_chain(inter_items, ritems, level, abs_sum, dist_resi, zero_dist, ctx, est, nxt, cbf_bits, prev, weight, scale):
    """the restatement of the two new calls fed with the downloaded levels and pixel-pass outputs"""
    rate = rrc.restate(level, ritems, abs_sum.reshape(-1), ctx, est, nxt)
    n = len(inter_items)
    chosen = rrc.choose(inter_items["tr"], abs_sum.reshape(n, -1), dist_resi.reshape(n, -1), zero_dist, rate["frac_bits"].reshape(n, -1), cbf_bits, prev,
                        weight, scale)
    return rate, chosen
