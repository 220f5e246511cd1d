#!/usr/bin/env python3
"""The rate half of the inter residual RD loop on the lists of tools/inter_resi_code_time.py (a 10-bit 3840x2160 4:2:0 picture, every CU as luma, Cb and
Cr items: "4K", every interior 16x16 CU, and "mix", 8 000 CUs whose shapes follow the committed call trace; each with one DCT-II slot per item and once
more with the four inter-EMT pairs as further slots of the luma items).  vvcgpu_inter_resi_code_batch runs first and leaves its level blocks on the
device; then, per list:
  pass    vvcgpu_inter_resi_code_batch alone (the pixel pass, for scale);
  rate    vvcgpu_resi_rate_batch on its 6 n level blocks with gate = abs_sum: one launch;
  chain   the pixel pass, the rate and vvcgpu_inter_resi_choose_batch back to back: three launches, nothing downloaded;
  copy    the device-to-host copy of the same level buffer into pinned memory: the step the rate entry removes, and the one alternative that exists where
          the reference's host estimator does not (it would follow the copy, on one core).
The rate and the compare are checked against the restatement (tests/resi_rate_cases.py) on the first 60 items of every list before anything is timed.
Times: device events around a whole run on the stream (the copy: a host clock around the copy and its synchronisation), 3 warm-up runs, then the median
and the spread of 9 runs, the four taking turns in one process.  The context rows and the model tables are those of tests/golden/resi_rate.npz."""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import inter_resi_code_chain  # noqa: E402
import inter_resi_code_time as irt  # noqa: E402
import pu_search_kit  # noqa: E402
import rd_pass_kit as kit  # noqa: E402
import resi_rate_cases as rrc  # noqa: E402
import resi_rate_chain as chain  # noqa: E402
from vvcsoftware_vtm_amd import ops  # noqa: E402

WARMUP, RUNS, CHECKED = 3, 9, 60


def main():
    rng = np.random.default_rng(47)                                        # the lists of tools/inter_resi_code_time.py: the same draws in the same order
    org, pred = irt.planes(rng)
    cus = kit.timing_lists(rng, irt.W, irt.H, (4, 8, 16, 32, 64))
    g = rrc.golden()
    M = chain.Model(g["est_bits"], g["next_state"])
    ctx = np.stack([g["ctx_before"][2], g["ctx_before"][len(g["ctx_before"]) - 2]])
    ctx_dev = kit.dev(ctx)
    print("list             items   blocks   levels MB   pass ms   rate ms (min..max)   chain ms (min..max)   copy ms (min..max)   copy / rate")
    for emt in (False, True):
        for name, w, h, px, py in cus:
            it, size = irt.build(w, h, px, py, emt)
            n = len(it)
            D = inter_resi_code_chain.Device(irt.BD, org, pred, it, size, size)
            resi, _, level = D.fresh()
            luma = (np.arange(n) % 3 == 0).astype(np.int8)
            ritems = chain.rate_items(it, luma, 0)
            ritems_dev = ops.struct_to_device(ritems)
            cbf_bits, prev, weight, scale = chain.chain_inputs(n, 3)
            cbf_dev, prev_dev, weight_dev = kit.dev(chain.signed(cbf_bits)), kit.dev(prev), kit.dev(weight)
            pinned = torch.empty(size, dtype=torch.int32).pin_memory()
            state = {}

            def pixel():
                state["pass"] = D.run_entry(resi, None, level, 0)
                return state["pass"]

            def rate():
                return ops.resi_rate_batch(level, ritems_dev, 6 * n, ctx_dev, M.est, M.nxt, state["pass"][0])

            def chained():
                abs_sum, dist_resi, _, zero_dist = pixel()
                frac, _ = ops.resi_rate_batch(level, ritems_dev, 6 * n, ctx_dev, M.est, M.nxt, abs_sum)
                return ops.inter_resi_choose_batch(D.items_dev, n, abs_sum, dist_resi, zero_dist, frac, cbf_dev, prev_dev, weight_dev, scale)

            def copy():
                pinned.copy_(level, non_blocking=True)
                torch.cuda.synchronize()

            # the check: the first items against the restatement, fed with the downloaded levels
            got = chained()
            frac, nsig = rate()
            torch.cuda.synchronize()
            abs_sum = state["pass"][0].cpu().numpy().view(np.uint32)
            k = min(CHECKED, n)
            want_rate, want_chosen = chain.want_chain(it[:k], ritems[:6 * k], level.cpu().numpy(), abs_sum[:k], state["pass"][1].cpu().numpy().view(np.uint64)[:k],
                                                      state["pass"][3].cpu().numpy().view(np.uint64)[:k], ctx, g["est_bits"], g["next_state"], cbf_bits[:k],
                                                      np.where(prev[:k] < k, prev[:k], -1), weight[:k], scale)
            assert np.array_equal(frac.cpu().numpy().view(np.uint64)[:6 * k], want_rate["frac_bits"]) and np.array_equal(nsig.cpu().numpy().view(np.uint32)[:6 * k], want_rate["num_sig"])
            assert np.array_equal(got[0].cpu().numpy()[:k], want_chosen["slot"]) and got[5].cpu().numpy()[:k].tobytes() == want_chosen["min_cost"].tobytes()
            blocks = int((abs_sum != rrc.U32_MAX).sum())

            def copy_ms():
                t0 = time.perf_counter()
                copy()
                return (time.perf_counter() - t0) * 1e3

            for _ in range(WARMUP):
                pixel(), rate(), chained(), copy()
            tp, tr, tc, ty = [], [], [], []
            for _ in range(RUNS):
                tp.append(pu_search_kit.events(pixel)[0]); tr.append(pu_search_kit.events(rate)[0]); tc.append(pu_search_kit.events(chained)[0])
                torch.cuda.synchronize()
                ty.append(copy_ms())
            med = lambda t: float(np.median(t))
            print("%-14s %7d %8d %11.1f %9.3f   %7.3f (%.3f..%.3f)   %8.3f (%.3f..%.3f)   %7.3f (%.3f..%.3f)   %11.2f"
                  % (name + (" +EMT" if emt else ""), n, blocks, size * 4 / 1e6, med(tp), med(tr), min(tr), max(tr), med(tc), min(tc), max(tc), med(ty), min(ty),
                     max(ty), med(ty) / med(tr)))


if __name__ == "__main__":
    main()
