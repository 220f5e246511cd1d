#!/usr/bin/env python3
"""The pixel pass of the intra RD loop (IntraSearch::xIntraCodingTUBlock, IntraSearch.cpp:1147-1316) of a 10-bit 3840x2160 picture, three candidate modes
per PU, every candidate into buffers of its own:
  4K      every interior 16x16 block of the picture;
  mix     about 8 000 PUs at random positions whose shapes follow the committed call trace (tests/golden/trace_ragop16_416x240_10b_q32.npz: the
          shapes of its pelop calls with sides 4..64), grouped by shape.
Random modes with the luma filter rule's decision, DCT-II, QP 32, sign hiding on, references gathered on the device beforehand.
  (a) the chained form, built from entries whose code the new entry does not alter: vvcgpu_intra_pred_batch, vvcgpu_resi_chain_runs_batch (both lists
      are grouped by shape), vvcgpu_dist_batch kind 2 -- three launches back to back, no host work between, descriptors uploaded outside the timed part;
  (b) vvcgpu_intra_tu_code_batch: one launch, the prediction never written.
The results of (a) and (b) are compared before anything is timed.  Times: device events around a whole run on the stream, 3 warm-up runs, then the median
and the spread of 9 runs, (a) and (b) alternating in one process.  The two lists and the row come from tests/rd_pass_kit.py."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import intra_mode_cand_cases as imc  # noqa: E402
import pu_search_kit  # noqa: E402
import rd_pass_kit as kit  # noqa: E402
from rd_pass_kit import dev  # noqa: E402
from vvcsoftware_vtm_amd import abi, ops  # noqa: E402

W, H, BD = 3840, 2160, 10
CANDS, QP = 3, 32 + 12
WARMUP, RUNS = 3, 9
rng = np.random.default_rng(43)


def build(w, h, px, py):
    """-> the descriptor arrays of the PUs' gathering and of the CANDS items per PU, grouped by shape"""
    order = np.lexsort((h, w))
    w, h, px, py = w[order], h[order], px[order], py[order]
    n = len(w)
    lens = np.array([sum(imc.ref_lengths(int(a), int(b))) + 1 for a, b in zip(w, h)])
    ref_off = np.concatenate([[0], np.cumsum(lens)[:-1]])
    fill = np.zeros(n, abi.INTRA_FILL_DESC)
    fill["rec_off"], fill["ref_off"], fill["rec_stride"], fill["w"], fill["h"], fill["unit_w"], fill["unit_h"] = py.astype(np.int64) * W + px, ref_off, W, w, h, 4, 4
    pu = np.repeat(np.arange(n), CANDS)
    iw, ih = w[pu].astype(np.int64), h[pu].astype(np.int64)
    m = len(pu)
    modes = rng.integers(0, imc.N_MODES, m)
    filt = np.array([imc.use_filtered(int(a), int(b), int(c)) for a, b, c in zip(iw, ih, modes)], np.int8)
    area = iw * ih
    off = np.concatenate([[0], np.cumsum(area)[:-1]])
    d = np.zeros(m, abi.INTRA_DESC)
    d["ref_off"], d["dst_off"], d["dst_stride"], d["w"], d["h"], d["mode"], d["filter_refs"] = ref_off[pu], off, iw, iw, ih, modes, filt
    t = np.zeros(m, abi.RC_DESC)
    t["org_off"], t["org_stride"] = fill["rec_off"][pu], W
    t["pred_off"], t["rec_off"], t["level_off"], t["pred_stride"], t["rec_stride"] = off, off, off, iw, iw
    t["w"], t["h"], t["intra_slice"], t["sign_hiding"], t["qp"] = iw, ih, 1, 1, QP
    dd = np.zeros(m, abi.DIST_DESC)
    dd["org_off"], dd["cur_off"], dd["org_stride"], dd["cur_stride"], dd["w"], dd["h"] = t["org_off"], off, W, iw, iw, ih
    runs = []
    for a, b in zip(iw, ih):
        if runs and runs[-1][0] == a and runs[-1][1] == b:
            runs[-1][2] += 1
        else:
            runs.append([int(a), int(b), 1])
    return fill, int(lens.sum()), d, t, dd, runs, int(area.sum())


def main():
    rec = pu_search_kit.texture(rng, H, W, BD, 0.0)
    org = np.clip(np.roll(rec, (1, -2), axis=(0, 1)).astype(np.int32) + rng.integers(-4, 5, (H, W)), 0, 1023).astype(np.int16)
    lists = kit.timing_lists(rng, W, H, imc.SIDES)
    drec, dorg, avail = dev(rec.reshape(-1)), dev(org.reshape(-1)), dev(np.ones(192, np.uint8))
    clp = (0, 1023)
    print("list        items   chain ms (min..max)   entry ms (min..max)   chain / entry   all-zero items")
    for name, w, h, px, py in lists:
        fill, nrefs, d, t, dd, runs, samples = build(w, h, px, py)
        m = len(d)
        refs = torch.zeros(nrefs, dtype=torch.int16, device="cuda")
        ops.intra_fill_refs_batch(drec, avail, refs, ops.struct_to_device(fill), len(fill), BD)
        dd_, dt, ddd = ops.struct_to_device(d), ops.struct_to_device(t), ops.struct_to_device(dd)
        pred = torch.zeros(samples, dtype=torch.int16, device="cuda")
        rec_a, rec_b = torch.zeros_like(pred), torch.zeros_like(pred)
        lev_a, lev_b = torch.zeros(samples, dtype=torch.int32, device="cuda"), torch.zeros(samples, dtype=torch.int32, device="cuda")

        def chained():
            ops.intra_pred_batch(refs, pred, dd_, m, clp)
            a = ops.resi_chain_runs_batch(dorg, pred, rec_a, lev_a, dt, m, runs, BD, clp)
            return a, ops.dist_batch(2, dorg, rec_a, ddd, m, BD)

        def entry():
            return ops.intra_tu_code_batch(refs, dd_, dorg, None, rec_b, lev_b, dt, m, None, 0, BD, clp)

        def check(oc, oe):
            (sa, da), (sb, nb, db, mb) = oc, oe
            assert torch.equal(rec_a, rec_b) and torch.equal(lev_a, lev_b) and torch.equal(sa, sb) and torch.equal(da, db), name
            nz = torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda"), (lev_b != 0).to(torch.int64).cumsum(0)])     # non-zero levels in front of each position
            ends = dev(t["level_off"] + t["w"].astype(np.int64) * t["h"])
            assert torch.equal(mb, dev(d["mode"].astype(np.int32))) and torch.equal(nb.to(torch.int64), nz[ends] - nz[dev(t["level_off"])]), name
            return int((nb == 0).sum())

        kit.time_row("%-10s %6d" % (name, m), chained, entry, check, WARMUP, RUNS)


if __name__ == "__main__":
    main()
