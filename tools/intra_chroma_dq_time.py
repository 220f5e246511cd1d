#!/usr/bin/env python3
"""The intra chroma mode pass under DepQuant 1 on the two lists of tools/intra_chroma_code_time.py (the 8x8 chroma PU under every interior 16x16 luma block
of a 10-bit 3840x2160 4:2:0 picture; 8 000 PUs with the trace's shapes halved, luma sides 8..64, so no chroma side is 2), six slots per PU, QP 32.  Three
records per PU: lambdas 60 / 90 / 700 and tables of tests/golden/depquant.npz in turn, the two Cr tables different.
  (a) the chain of the entries that existed before (tests/intra_chroma_dq_chain.py): intra_fill_refs_batch x 2, intra_pred_batch, cclm_pred_batch,
      intra_tu_code_dq_batch (PRED_GIVEN) for Cb, the download of its abs_sum, the host's choice and upload of the Cr records, intra_tu_code_dq_batch for
      Cr -- the download and the host work are inside the timed part: that is what the entry replaces;
  (b) vvcgpu_intra_chroma_code_dq_batch: references gathered inside, not written; no prediction written; its workspace allocated outside the timed part.
The results of (a) and (b) are compared before anything is timed.  Times: device events around a whole run on the stream, 3 warm-up runs, then the median and
the spread of 9 runs, (a) and (b) alternating in one process.  --profile: three runs of (b) per list and nothing else, for a kernel trace
(chroma_dq_front_kernel, depquant_listed_kernel twice -- the trellis launch that the DepQuant entries share, depquant.hip --, chroma_dq_select_kernel between
them, chroma_dq_back_kernel)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import intra_chroma_code_time as cct  # noqa: E402
import intra_chroma_dq_chain as chain  # noqa: E402
import inter_resi_dq_cases as dqc  # noqa: E402
import pu_search_kit  # noqa: E402
import rd_pass_kit as kit  # noqa: E402
from rd_pass_kit import dev  # noqa: E402
from vvcsoftware_vtm_amd import abi, ops  # noqa: E402

W, H, BD, CW, CH, rng = cct.W, cct.H, cct.BD, cct.CW, cct.CH, cct.rng
LAMBDAS = (60.0, 90.0, 700.0)


def main():
    profile = "--profile" in sys.argv
    luma = pu_search_kit.texture(rng, H, W, BD, 0.0)                            # the planes and the lists of intra_chroma_code_time.py, in its order of draws
    ds = luma[::2, ::2].astype(np.float64)
    rec = np.stack([np.clip(np.rint(205 + 0.55 * ds + rng.normal(0, 7, ds.shape)), 0, 1023), np.clip(np.rint(818 - 0.45 * ds + rng.normal(0, 7, ds.shape)), 0, 1023)]).astype(np.int16)
    org = np.clip(np.roll(rec, (1, -1), axis=(1, 2)).astype(np.int32) + rng.integers(-12, 13, rec.shape), 0, 1023).astype(np.int16)
    lists = kit.timing_lists(rng, CW, CH, (8, 16, 32, 64), chroma=True)
    drec, dorg, dluma, avail = dev(rec.reshape(-1)), dev(org.reshape(-1)), dev(luma.reshape(-1)), dev(np.ones(192, np.uint8))
    clp = (0, 1023)
    rates = dqc.shared_rates()
    drates = ops.struct_to_device(rates)
    if not profile:
        print("list        PUs    items   chain ms (min..max)   entry ms (min..max)   chain / entry   all-zero items")
    for name, w, h, px, py in lists:
        pus, fill, runs, nrefs, samples = cct.build(w, h, px, py)
        n = len(pus)
        dq = np.zeros(3 * n, abi.INTER_RESI_DQ)
        q = np.arange(n)
        for j in range(3):
            dq["lambda"][j::3], dq["rates_idx"][j::3] = LAMBDAS[j], (q + (0, 3, 5)[j]) % len(rates)
        refs = torch.zeros(nrefs, dtype=torch.int16, device="cuda")
        pred = torch.zeros(samples, dtype=torch.int16, device="cuda")
        rec_a, rec_b = torch.zeros_like(pred), torch.zeros_like(pred)
        lev_a, lev_b = torch.zeros(samples, dtype=torch.int32, device="cuda"), torch.zeros(samples, dtype=torch.int32, device="cuda")
        dpus, dfill, ddq = ops.struct_to_device(pus), ops.struct_to_device(fill), ops.struct_to_device(dq)
        ws = ops.intra_chroma_code_dq_workspace(samples, n)

        def entry():
            return ops.intra_chroma_code_dq_batch(dorg, dpus, ddq, n, runs, drates, len(rates), rec_b, lev_b, None, (drec, avail, dfill), dluma, None, 0, BD, clp, ws)

        if profile:
            for _ in range(3):
                entry()
            torch.cuda.synchronize()
            continue
        ch = chain.DqChain(pus, fill, dq, rates, BD, clp, drec, avail, dluma, dorg, refs, pred, rec_a, lev_a)
        ch.gather()
        ch.repack()

        def check(oc, oe):
            (sa, da), (sb, db) = oc, oe
            assert torch.equal(rec_a, rec_b) and torch.equal(lev_a, lev_b), name
            assert torch.equal(sa, sb.reshape(-1)) and torch.equal(da, db.reshape(-1)), name     # six slots in use: the items are the entry's, in its order
            return int((sb == 0).sum())

        kit.time_row("%-10s %6d %7d" % (name, n, 12 * n), ch.run, entry, check, cct.WARMUP, cct.RUNS)


if __name__ == "__main__":
    main()
