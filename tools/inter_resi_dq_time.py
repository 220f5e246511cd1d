#!/usr/bin/env python3
"""The inter residual pixel pass under DepQuant 1 on the two lists of tools/inter_resi_code_time.py (a 10-bit 3840x2160 4:2:0 picture, every CU as luma, Cb and
Cr items: every interior 16x16 CU; 8 000 CUs whose shapes follow the committed call trace, here with luma sides 8..64 so that no chroma block has a side of
2), each with one DCT-II slot per item, then once more with the four inter-EMT pairs as further slots of the luma items.  Lambda 60 and eight of the rate
tables of tests/golden/depquant.npz, one per item in turn.
  (a) the chained form (tests/inter_resi_dq_chain.py) from entries whose results the new entry does not alter: pelop_batch subtract, tr_fwd_batch,
      depquant_batch, dequant_tr_inv_batch (dep_quant = 1), dist_batch twice, pelop_batch reco, dist_batch -- eight launches back to back;
  (b) vvcgpu_inter_resi_code_dq_batch with WRITE_REC off: three launches, the workspace allocated outside the timed part.
The results of (a) and (b) are compared before anything is timed.  Times: device events around a whole run on the stream, 3 warm-up runs, then the median
and the spread of 9 runs, (a) and (b) alternating in one process.
--profile: no timing, five runs of (b) per list -- the run to put under `rocprofv3 --kernel-trace --stats` for the split into inter_resi_dq_front_kernel,
inter_resi_dq_trellis_kernel and inter_resi_dq_back_kernel."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import inter_resi_code_time as sibling  # noqa: E402
import inter_resi_dq_cases as dqc  # noqa: E402
import inter_resi_dq_chain as chain  # noqa: E402
import pu_search_kit as kit  # noqa: E402
from vvcsoftware_vtm_amd import abi, shape_mix  # noqa: E402

W, H, BD = sibling.W, sibling.H, sibling.BD
LAMBDA = 60.0
WARMUP, RUNS = 3, 9
rng = np.random.default_rng(48)


def main():
    profile = "--profile" in sys.argv
    luma = kit.texture(rng, H, W, BD, 0.0)
    planes = [luma, np.ascontiguousarray(luma[0::2, 0::2]), np.ascontiguousarray(luma[1::2, 1::2])]
    org = np.concatenate([p.reshape(-1) for p in planes])
    pred = np.concatenate([np.clip(np.roll(p, (1, -2), axis=(0, 1)).astype(np.int32) + rng.integers(-4, 5, p.shape), 0, 1023).astype(np.int16).reshape(-1) for p in planes])
    hist, _ = shape_mix.load_trace()
    sides = (8, 16, 32, 64)
    sig = shape_mix.signatures(hist, "pelop", lambda w, h, a, b, c: a == 0 and w in sides and h in sides)
    mix = np.array([(int(w), int(h)) for w, h in sig[rng.choice(len(sig), 8000, p=sig[:, 5] / sig[:, 5].sum()), :2]])
    bx, by = np.meshgrid(np.arange(1, W // 16 - 2), np.arange(1, H // 16 - 2))
    g = np.stack([bx.ravel() * 16, by.ravel() * 16], 1)
    cus = [("4K 16x16", np.full(len(g), 16), np.full(len(g), 16), g[:, 0], g[:, 1]),
           ("trace mix", mix[:, 0], mix[:, 1], rng.integers(1, (W - 160) // 4, len(mix)) * 4, rng.integers(1, (H - 160) // 4, len(mix)) * 4)]
    rates = dqc.shared_rates(8)
    if not profile:
        print("list             items   slots   chain ms (min..max)   entry ms (min..max)   chain / entry   all-zero slots")
    for emt in (False, True):
        for name, w, h, px, py in cus:
            it, size = sibling.build(w, h, px, py, emt)
            assert (it["level_off"] % 16 == 0).all()
            dq = np.zeros(len(it), abi.INTER_RESI_DQ)
            dq["lambda"], dq["rates_idx"], dq["luma"] = LAMBDA, np.arange(len(it)) % len(rates), np.arange(len(it)) % 3 == 0
            D = chain.Device(BD, org, pred, it, dq, rates, size, size)
            rb, _, lb = D.fresh()

            def entry():
                return D.run_entry(rb, None, lb, 0)

            if profile:
                for _ in range(5):
                    entry()
                torch.cuda.synchronize()
                continue
            C = chain.Chain(D)
            ra, ca, la = D.fresh()

            def chained():
                return C.run(ra, ca, la)

            oc, oe = chained(), entry()
            torch.cuda.synchronize()
            assert C.same(oc, oe) and torch.equal(ra, rb) and torch.equal(la, lb), name
            ta, tb = kit.times_of_alternating((chained, entry), WARMUP - 1, RUNS)   # the comparison above was the first warm-up run
            ma, mb = float(np.median(ta)), float(np.median(tb))
            print("%-14s %7d %7d   %8.3f (%.3f..%.3f)   %8.3f (%.3f..%.3f)   %13.2f   %d" %
                  (name + (" +EMT" if emt else ""), len(it), C.m, ma, min(ta), max(ta), mb, min(tb), max(tb), ma / mb, int((oc[0] == 0).sum())))


if __name__ == "__main__":
    main()
