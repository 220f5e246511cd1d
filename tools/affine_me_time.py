#!/usr/bin/env python3
"""Whole affine motion searches at 4K, every 16 / 32 / 64 / 128 square PU of a 3840x2160 plane (originals = the affine prediction with "true" vectors
plus noise, starts = the truth displaced, so the iterations run):
  (a) the loop over vvcgpu_affine_me_iter_batch: per iteration one call for the PUs still searching, a synchronise, the download of 49 sums and a
      distortion per PU, a vectorised numpy solve / vector update / cost on the host, the upload of the new vectors;
  (b) vvcgpu_affine_me_batch: one call, one synchronise, the download of the results.
Both start from the items on the host and end with the results on the host.  The final vectors, bits and costs of (a) and (b) are compared before
anything is timed; (a) and (b) alternate in one process in windows of about 0.4 s each, both run twice for the spread; times are host clocks per run that
end in a synchronise.  steps x iter: the mean number of evaluated predictions times the device time of one vvcgpu_affine_me_iter_batch over all PUs."""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from pu_search_kit import eg_bits  # noqa: E402
from vvcsoftware_vtm_amd import abi, ops  # noqa: E402

W, H, bd, M = 3840, 2160, 10, 144
PW = W + 2 * M
LAMBDA, AFFINE_TYPE = 37.5, 1
WINDOW_MS = 400.0
rng = np.random.default_rng(11)


def texture(h, w):
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    a = 0.5 + 0.22 * np.sin(x / 9.0 + y / 23.0) + 0.18 * np.cos(y / 7.0 - x / 31.0) + 0.08 * np.sin((x + 2 * y) / 3.5)
    return np.clip(np.rint(a * 1023 + rng.normal(0, 5.0, (h, w))), 0, 1023).astype(np.int16)


def quant(d):
    """(int)(d * 4 + SIGN(d) * 0.5) << 2 with the x86 conversion (0x80000000 for NaN / out of range), vectorised"""
    with np.errstate(all="ignore"):
        r = d * 4 + np.where(d >= 0, 0.5, -0.5)
        bad = ~((r >= -2147483648.0) & (r < 2147483648.0))
        q = np.where(bad, -2147483648, np.trunc(np.where(bad, 0.0, r))).astype(np.int64)
    q = (q << 2) & 0xFFFFFFFF
    return np.where(q & 0x80000000, q - (1 << 32), q)


def solve(coef, order):
    """solveEqual (InterSearch.cpp:3102-3179) for a batch: coef [n, 7, 7] int64 -> parameters [n, order]"""
    n = coef.shape[0]
    m = coef[:, 1:order + 1, :order + 1].astype(np.float64)          # row r - 1 = dEqualCoeff[r]
    alive = np.ones(n, bool)
    ar = np.arange(n)
    with np.errstate(all="ignore"):
        for i in range(order - 1):                                      # reference's i = 1 .. order - 1, column i - 1
            a = np.abs(m[:, i:, i])
            a[:, 1:] = np.where(np.isnan(a[:, 1:]), -1.0, a[:, 1:])     # fabs(x) > temp is false for NaN
            a[:, 0] = np.where(np.isnan(a[:, 0]), np.inf, a[:, 0])
            idx = i + np.argmax(a, axis=1)                              # the first maximum: strict '>' in row order
            tmp = m[ar, i].copy()
            m[ar, i] = m[ar, idx]
            m[ar, idx] = tmp
            alive &= m[:, i, i] != 0.
            for j in range(i + 1, order):
                f = m[:, j, i].copy()
                for k in range(i + 1, order + 1):
                    m[:, j, k] = m[:, j, k] - m[:, i, k] * f / m[:, i, i]
        alive &= m[:, order - 1, order - 1] != 0.
        para = np.zeros((n, order))
        para[:, order - 1] = m[:, order - 1, order] / m[:, order - 1, order - 1]
        for i in range(order - 2, -1, -1):
            alive &= m[:, i, i] != 0.
            temp = np.zeros(n)
            for j in range(i + 1, order):
                temp = temp + m[:, i, j] * para[:, j]
            para[:, i] = (m[:, i, order] - temp) / m[:, i, i]
    para[~alive] = 0.
    return para


def deltas(coef, six, B):
    """equation sums -> quantised vector deltas [n, 3, 2] (:3609-3633)"""
    out = np.zeros((coef.shape[0], 3, 2), np.int64)
    with np.errstate(all="ignore"):
        for s in (0, 1):
            g = six == s
            if not g.any():
                continue
            a = solve(coef[g], 6 if s else 4)
            if s:
                d = [a[:, 0], a[:, 2], a[:, 1] * B + a[:, 0], a[:, 3] * B + a[:, 2], a[:, 4] * B + a[:, 0], a[:, 5] * B + a[:, 2]]
            else:
                d = [a[:, 0], a[:, 2], a[:, 1] * B + a[:, 0], -a[:, 3] * B + a[:, 2]]
            o = np.zeros((a.shape[0], 3, 2), np.int64)
            for k, v in enumerate(d):
                o[:, k // 2, k % 2] = quant(v)
            out[g] = o
    return out


def clip_mv(mv, pos):
    """clipMv of [n, k, 2] vectors in 1/16 units"""
    lo = np.stack([(-128 - 8 - pos[:, 0] + 1) << 4, (-128 - 8 - pos[:, 1] + 1) << 4], 1)[:, None, :]
    hi = np.stack([(W + 8 - pos[:, 0] - 1) << 4, (H + 8 - pos[:, 1] - 1) << 4], 1)[:, None, :]
    return np.minimum(hi, np.maximum(lo, mv))


def costs(items, mv, had):
    six = items["pu"]["six_param"] != 0
    mvp = items["mvp"].astype(np.int64)
    pred = mvp.copy()
    pred[:, 1:] += (mv[:, 0] - mvp[:, 0])[:, None, :]
    b = eg_bits((mv >> 2) - (pred >> 2)).sum(axis=2)                    # [n, 3]
    bits = items["bits"].astype(np.int64) + b[:, 0] + b[:, 1] + np.where(six, b[:, 2], 0)
    weight = np.where(items["half_weight"] != 0, 0.5, 1.0)
    return bits, (np.floor(weight * had.astype(np.float64)) + np.floor(LAMBDA * bits)).astype(np.int64)


def host_loop(org, ref, items, B, pred_ws):
    """(a): -> (AFFINE_ME_RESULT records, calls made, PU-iterations run)"""
    n = len(items)
    six = items["pu"]["six_param"] != 0
    pos = np.stack([items["pu"]["pos_x"], items["pu"]["pos_y"]], 1).astype(np.int64)
    hw = items["half_weight"] != 0
    limit = np.where(six, np.where(hw, 3, 4), np.where(hw, 3, 5)) if AFFINE_TYPE else np.where(hw, 5, 7)
    cur = items["pu"]["mv"][:, 0].astype(np.int64)
    c = clip_mv(cur, pos)
    cur = np.where(six[:, None, None] | (np.arange(3) < 2)[None, :, None], c, cur)
    res = np.zeros(n, abi.AFFINE_ME_RESULT)
    active = np.arange(n)
    it = np.zeros(n, abi.AFFINE_ITER)
    it["pu"], it["org_off"], it["org_stride"] = items["pu"], items["org_off"], items["org_stride"]
    nsb = (B // 4) ** 2
    calls = work = 0
    step = 0
    while active.size:
        a = it[active]
        a["pu"]["mv"][:, 0] = cur[active]
        k = active.size
        a["pu"]["dst_off"], a["pu"]["dst_stride"], a["pu"]["first_desc"] = np.arange(k) * B * B, B, np.arange(k) * nsb
        coef, dist = ops.affine_me_iter_batch(org, ref, pred_ws, ops.struct_to_device(a), k, k * nsb, 1, W, H, (M, M), PW, bd, (0, 1023))
        torch.cuda.synchronize()
        coef, had = coef.cpu().numpy(), dist.cpu().numpy()
        calls += 1
        work += k
        bits, cost = costs(items[active], cur[active], had)
        if step == 0:
            res["mv"], res["bits"], res["cost"], res["steps"] = cur, bits, cost, 1
        else:
            res["steps"][active] += 1
            better = cost.astype(np.uint64) < res["cost"][active]
            w = active[better]
            res["mv"][w], res["bits"][w], res["cost"][w] = cur[w], bits[better], cost[better]
        go = step < limit[active]
        dl = deltas(coef, six[active], B)
        nz = (dl != 0).any(axis=2)
        go &= nz[:, 0] | nz[:, 1] | (six[active] & nz[:, 2])
        act2 = active[go]
        v = cur[act2] + dl[go]
        v = ((v + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)
        v = np.clip(v, -32768, 32767)
        v = np.where(v >= 0, (v + 2) >> 2, -((-v + 2) >> 2)) * 4
        v = clip_mv(v, pos[act2])
        cur[act2] = np.where(six[act2][:, None, None] | (np.arange(3) < 2)[None, :, None], v, cur[act2])
        active = act2
        step += 1
    return res, calls, work


def one_call(org, ref, items, cfg):
    r, _ = ops.affine_me_batch(org, ref, ops.struct_to_device(items), len(items), cfg, want_trace=False)
    torch.cuda.synchronize()
    return r.cpu().numpy().view(abi.AFFINE_ME_RESULT)


def clock(fn, reps=1):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3 / reps


def main():
    refn = texture(H, W)
    ref = torch.from_numpy(np.pad(refn, M, mode="edge")).cuda()
    cfg = ops.affine_me_cfg(LAMBDA, W, H, (M, M), PW, bd, (0, 1023), AFFINE_TYPE)
    print("whole affine searches at %dx%d, %d-bit, lambda %.1f, affine_type %d; times in ms" % (W, H, bd, LAMBDA, AFFINE_TYPE))
    print("%-8s %7s %6s %9s %9s %9s %9s %7s %12s" % ("PU", "PUs", "steps", "(a) run1", "(a) run2", "(b) run1", "(b) run2", "(a)/(b)", "steps x iter"))
    for B in (16, 32, 64, 128):
        xs, ys = np.arange(0, W - B + 1, B), np.arange(0, H - B + 1, B)
        gx, gy = (v.reshape(-1) for v in np.meshgrid(xs, ys))
        n, nsb = gx.size, (B // 4) ** 2
        six = rng.integers(0, 2, n)
        t = rng.integers(-24, 25, (n, 1, 2)) * 4
        true = np.concatenate([t, t + rng.integers(-6, 7, (n, 2, 2)) * 4], 1)
        true[:, 2] = np.where(six[:, None] != 0, true[:, 2], np.stack([true[:, 0, 0] - (true[:, 1, 1] - true[:, 0, 1]), true[:, 0, 1] + (true[:, 1, 0] - true[:, 0, 0])], 1))
        pus = np.zeros(n, abi.AFFINE_PU)
        pus["pos_x"], pus["pos_y"], pus["w"], pus["h"], pus["six_param"] = gx, gy, B, B, six
        pus["mv"][:, 0] = true
        pus["dst_off"], pus["dst_stride"], pus["first_desc"] = np.arange(n) * B * B, B, np.arange(n) * nsb
        pred_ws = torch.zeros(n * B * B, dtype=torch.int16, device="cuda")
        ops.affine_pred_batch(ref, None, pred_ws, ops.struct_to_device(pus), n, n * nsb, 0, W, H, (M, M), PW, PW, bd, (0, 1023))
        org = torch.from_numpy(refn.copy()).cuda()
        blocks = pred_ws.reshape(ys.size, xs.size, B, B).permute(0, 2, 1, 3).reshape(ys.size * B, xs.size * B)
        noise = torch.from_numpy(rng.integers(-4, 5, tuple(blocks.shape)).astype(np.int16)).cuda()
        org[:ys.size * B, :xs.size * B] = torch.clamp(blocks + noise, 0, 1023)
        items = np.zeros(n, abi.AFFINE_ME_ITEM)
        items["pu"]["pos_x"], items["pu"]["pos_y"], items["pu"]["w"], items["pu"]["h"], items["pu"]["six_param"] = gx, gy, B, B, six
        start = true + rng.integers(-6, 7, (n, 3, 2)) * 4
        items["pu"]["mv"][:, 0] = start
        items["mvp"] = start + rng.integers(-3, 4, (n, 3, 2)) * 4
        items["org_off"], items["org_stride"], items["bits"] = gy * W + gx, W, rng.integers(0, 9, n)
        items["half_weight"] = rng.integers(0, 4, n) == 0

        ra, calls, work = host_loop(org, ref, items, B, pred_ws)
        rb = one_call(org, ref, items, cfg)
        for f in ("mv", "bits", "cost", "steps"):
            assert np.array_equal(ra[f], rb[f]), (B, f, np.nonzero((ra[f] != rb[f]).reshape(n, -1).any(axis=1))[0][:8])
        for _ in range(2):                                                # warm-up of both
            host_loop(org, ref, items, B, pred_ws)
            one_call(org, ref, items, cfg)
        fa, fb = (lambda: host_loop(org, ref, items, B, pred_ws)), (lambda: one_call(org, ref, items, cfg))
        ra_, rb_ = max(3, int(WINDOW_MS / clock(fa))), max(20, int(WINDOW_MS / clock(fb)))       # windows of about WINDOW_MS each
        a1, b1, a2, b2 = clock(fa, ra_), clock(fb, rb_), clock(fa, ra_), clock(fb, rb_)
        # one fused iteration over all PUs of the size (device time of the three launches of vvcgpu_affine_me_iter_batch)
        it = np.zeros(n, abi.AFFINE_ITER)
        it["pu"], it["org_off"], it["org_stride"] = items["pu"], items["org_off"], items["org_stride"]
        it["pu"]["dst_off"], it["pu"]["dst_stride"], it["pu"]["first_desc"] = np.arange(n) * B * B, B, np.arange(n) * nsb
        dit = ops.struct_to_device(it)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ops.affine_me_iter_batch(org, ref, pred_ws, dit, n, n * nsb, 1, W, H, (M, M), PW, bd, (0, 1023))
        torch.cuda.synchronize()
        e0.record()
        for _ in range(10):
            ops.affine_me_iter_batch(org, ref, pred_ws, dit, n, n * nsb, 1, W, H, (M, M), PW, bd, (0, 1023))
        e1.record()
        torch.cuda.synchronize()
        iter_ms = e0.elapsed_time(e1) / 10
        steps = rb["steps"].mean()
        print("%-8s %7d %6.2f %9.2f %9.2f %9.3f %9.3f %7.1f %12.2f" % ("%dx%d" % (B, B), n, steps, a1, a2, b1, b2, min(a1, a2) / max(b1, b2), steps * iter_ms),
              flush=True)


if __name__ == "__main__":
    main()
