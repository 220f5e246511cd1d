#!/usr/bin/env python3
"""The pixel pass of the intra RD loop under DepQuant 1 on the two lists of tools/intra_tu_code_time.py (a 10-bit 3840x2160 picture, three candidate modes per
PU, every candidate into buffers of its own: every interior 16x16 block; about 8 000 PUs whose shapes follow the committed call trace).  Random modes with
the luma filter rule's decision, DCT-II, QP 32, lambda 60 and eight of the rate tables of tests/golden/depquant.npz, one per item in turn; references
gathered on the device beforehand.
  (a) the chained form (tests/intra_tu_dq_chain.py) from entries whose results the new entry does not alter: intra_pred_batch, pelop_batch subtract,
      tr_fwd_batch, depquant_batch, dequant_tr_inv_batch (dep_quant = 1), pelop_batch reco, dist_batch -- seven launches back to back, descriptors
      uploaded outside the timed part;
  (b) vvcgpu_intra_tu_code_dq_batch with WRITE_PRED off: three launches, the workspace allocated outside the timed part.
The results of (a) and (b) are compared before anything is timed.  Times: device events around a whole run on the stream, 3 warm-up runs, then the median
and the spread of 9 runs, (a) and (b) alternating in one process.
--ts: the transform-skip candidate instead (VVCGPU_INTRA_TU_DQ_TS): at every PU position of the 4K list a 4x4 PU, per candidate mode a DCT-II item and the
skip item behind it (tr_hor = 3) -- checkTransformSkip of xRecurIntraCodingLumaQT.  (a) is the same chain (vvcgpu_tr_fwd_batch and
vvcgpu_dequant_tr_inv_batch serve tr_hor = 3; the prediction is formed for both items), (b) the entry with the flag.
--profile: no timing, five runs of (b) per list -- the run to put under `rocprofv3 --kernel-trace --stats` for the split into intra_tu_dq_front_kernel,
depquant_listed_kernel (the trellis launch that the DepQuant entries share, depquant.hip) and intra_tu_dq_back_kernel.
The planes and build are the sibling's; the lists and the row come from tests/rd_pass_kit.py."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import intra_mode_cand_cases as imc  # noqa: E402
import intra_tu_code_time as sibling  # noqa: E402
import intra_tu_dq_cases as tdq  # noqa: E402
import intra_tu_dq_chain as chain  # noqa: E402
import pu_search_kit  # noqa: E402
import rd_pass_kit as kit  # noqa: E402
from rd_pass_kit import dev  # noqa: E402
from vvcsoftware_vtm_amd import abi, ops  # noqa: E402

W, H, BD = sibling.W, sibling.H, sibling.BD
LAMBDA = 60.0
rng = np.random.default_rng(49)


def main():
    profile, ts = "--profile" in sys.argv, "--ts" in sys.argv
    rec = pu_search_kit.texture(rng, H, W, BD, 0.0)
    org = np.clip(np.roll(rec, (1, -2), axis=(0, 1)).astype(np.int32) + rng.integers(-4, 5, (H, W)), 0, 1023).astype(np.int16)
    lists = kit.timing_lists(rng, W, H, imc.SIDES)
    if ts:                                                                   # the 4K list's positions as 4x4 PUs
        _, w, _, px, py = lists[0]
        lists = [("4K 4x4 +TS", np.full_like(w, 4), np.full_like(w, 4), px, py)]
    drec, dorg, avail = dev(rec.reshape(-1)), dev(org.reshape(-1)), dev(np.ones(192, np.uint8))
    rates = tdq.shared_rates(8)
    drates = ops.struct_to_device(rates)
    clp = (0, 1023)
    if not profile:
        print("list        items   chain ms (min..max)   entry ms (min..max)   chain / entry   all-zero items")
    for name, w, h, px, py in lists:
        fill, nrefs, d, t, _, _, samples = sibling.build(w, h, px, py)
        if ts:                                                               # every item twice, buffers of its own each: DCT-II, then the skip item
            d, t = np.repeat(d, 2), np.repeat(t, 2)
            off = 16 * np.arange(len(d))
            d["dst_off"], t["pred_off"], t["rec_off"], t["level_off"], samples = off, off, off, off, 16 * len(d)
            t["tr_hor"][1::2] = abi.TSKIP
        m = len(d)
        assert (t["level_off"] % 16 == 0).all()
        dq = np.zeros(m, abi.INTER_RESI_DQ)
        dq["lambda"], dq["rates_idx"], dq["luma"] = LAMBDA, np.arange(m) % len(rates), 1
        refs = torch.zeros(nrefs, dtype=torch.int16, device="cuda")
        ops.intra_fill_refs_batch(drec, avail, refs, ops.struct_to_device(fill), len(fill), BD)
        dd_, dt, ddq = ops.struct_to_device(d), ops.struct_to_device(t), ops.struct_to_device(dq)
        pred_a = torch.zeros(samples, dtype=torch.int16, device="cuda")
        rec_a, rec_b = torch.zeros_like(pred_a), torch.zeros_like(pred_a)
        lev_a, lev_b = torch.zeros(samples, dtype=torch.int32, device="cuda"), torch.zeros(samples, dtype=torch.int32, device="cuda")
        ws = ops.intra_tu_code_dq_workspace(samples, m)

        def entry():
            return chain.run_entry(refs, dd_, dorg, None, rec_b, lev_b, dt, ddq, m, drates, len(rates), None, abi.INTRA_TU_DQ_TS if ts else 0, BD, clp, ws)

        if profile:
            for _ in range(5):
                entry()
            torch.cuda.synchronize()
            continue
        C = chain.Chain(d, t, dq, drates, samples, BD, refs, dorg)

        def chained():
            return C.run(pred_a, rec_a, lev_a)

        def check(oc, oe):
            (sa, da), (sb, nb, db, mb) = oc, oe
            assert torch.equal(rec_a, rec_b) and torch.equal(lev_a, lev_b) and torch.equal(sa, sb) and torch.equal(da, db), name
            assert torch.equal(mb, dev(d["mode"].astype(np.int32))) and torch.equal(nb == 0, sb == 0), name
            return int((sb == 0).sum())

        kit.time_row("%-10s %6d" % (name, m), chained, entry, check, sibling.WARMUP, sibling.RUNS)


if __name__ == "__main__":
    main()
