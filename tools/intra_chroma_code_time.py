#!/usr/bin/env python3
"""The intra chroma mode pass (IntraSearch::estIntraPredChromaQT, IntraSearch.cpp:704-852: xIntraCodingTUBlock for Cb and Cr per candidate mode) of a 10-bit
3840x2160 4:2:0 picture, six candidate slots per PU (planar / vertical / horizontal / DC with the VDIA substitution, LM in slot 4, a random DM), every
candidate into buffers of its own:
  4K      the 8x8 chroma PU under every interior 16x16 luma block of the picture;
  mix     8 000 PUs at random positions whose shapes are the PU shapes of the committed call trace (tests/golden/trace_ragop16_416x240_10b_q32.npz: the
          shapes of its pelop calls) halved; luma sides 8..64, i.e. chroma sides 4..32 -- the chain's last entry takes no 2-sample side.
QP 32, sign hiding on, every neighbour available.
  (a) the chain of the entries that existed before (tests/intra_chroma_code_chain.py): vvcgpu_intra_fill_refs_batch for Cb and for Cr,
      vvcgpu_intra_pred_batch, vvcgpu_cclm_pred_batch, vvcgpu_intra_tu_code_batch with PRED_GIVEN -- five launches back to back, no host work between;
      descriptors uploaded and the neighbours repacked into nb_base outside the timed part;
  (b) vvcgpu_intra_chroma_code_batch: references gathered inside, not written; no prediction written.
The results of (a) and (b) are compared before anything is timed.  Times: device events around a whole run on the stream, 3 warm-up runs, then the median
and the spread of 9 runs, (a) and (b) alternating in one process.  The two lists and the row come from tests/rd_pass_kit.py."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import intra_chroma_code_chain as chain  # noqa: E402
import pu_search_kit  # noqa: E402
import rd_pass_kit as kit  # noqa: E402
from rd_pass_kit import dev  # noqa: E402
from vvcsoftware_vtm_amd import abi, ops  # noqa: E402

W, H, BD = 3840, 2160, 10
CW, CH = W // 2, H // 2
QP = 32 + 12
WARMUP, RUNS = 3, 9
rng = np.random.default_rng(47)


def build(w, h, px, py):
    """-> (pus, fill, runs, reference samples, candidate samples) of chroma PUs of w x h at (px, py), grouped by shape"""
    order = np.lexsort((h, w))
    w, h, px, py = (v[order].astype(np.int64) for v in (w, h, px, py))
    n = len(w)
    T, L = chain.ref_lengths(w, h)
    lens = np.repeat(T + L + 1, 2)
    ref_off = np.concatenate([[0], np.cumsum(lens)[:-1]]).reshape(-1, 2)
    area = 12 * w * h
    cand = np.concatenate([[0], np.cumsum(area)[:-1]])
    pus = np.zeros(n, abi.INTRA_CHROMA_PU)
    fill = np.zeros(2 * n, abi.INTRA_FILL_DESC)
    for c in range(2):
        pus["org_off"][:, c] = c * CW * CH + py * CW + px
        pus["ref_off"][:, c] = ref_off[:, c]
        f = fill[c::2]
        f["rec_off"], f["ref_off"], f["rec_stride"], f["w"], f["h"], f["unit_w"], f["unit_h"] = c * CW * CH + py * CW + px, ref_off[:, c], CW, w, h, 2, 2
    pus["luma_off"], pus["luma_stride"], pus["org_stride"], pus["cand_off"], pus["level_off"] = 2 * py * W + 2 * px, W, CW, cand, cand
    pus["qp"], pus["w"], pus["h"], pus["above_avail"], pus["left_avail"], pus["intra_slice"], pus["sign_hiding"] = QP, w, h, 1, 1, 1, 1
    dm = rng.integers(0, 67, n)
    base = np.array([0, 50, 18, 1])
    pus["mode"][:, :4] = np.where(base[None, :] == dm[:, None], 66, base[None, :])
    pus["mode"][:, 4], pus["mode"][:, 5] = abi.INTRA_CHROMA_LM, dm
    runs = []
    for a, b in zip(w, h):
        if runs and runs[-1][0] == a and runs[-1][1] == b:
            runs[-1][2] += 1
        else:
            runs.append([int(a), int(b), 1])
    return pus, fill, runs, int(lens.sum()), int(area.sum())


def main():
    luma = pu_search_kit.texture(rng, H, W, BD, 0.0)
    ds = luma[::2, ::2].astype(np.float64)
    rec = np.stack([np.clip(np.rint(205 + 0.55 * ds + rng.normal(0, 7, ds.shape)), 0, 1023), np.clip(np.rint(818 - 0.45 * ds + rng.normal(0, 7, ds.shape)), 0, 1023)]).astype(np.int16)
    org = np.clip(np.roll(rec, (1, -1), axis=(1, 2)).astype(np.int32) + rng.integers(-12, 13, rec.shape), 0, 1023).astype(np.int16)
    lists = kit.timing_lists(rng, CW, CH, (8, 16, 32, 64), chroma=True)
    drec, dorg, dluma, avail = dev(rec.reshape(-1)), dev(org.reshape(-1)), dev(luma.reshape(-1)), dev(np.ones(192, np.uint8))
    clp = (0, 1023)
    print("list        PUs    items   chain ms (min..max)   entry ms (min..max)   chain / entry   all-zero items")
    for name, w, h, px, py in lists:
        pus, fill, runs, nrefs, samples = build(w, h, px, py)
        n = len(pus)
        refs = torch.zeros(nrefs, dtype=torch.int16, device="cuda")
        pred = torch.zeros(samples, dtype=torch.int16, device="cuda")
        rec_a, rec_b = torch.zeros_like(pred), torch.zeros_like(pred)
        lev_a, lev_b = torch.zeros(samples, dtype=torch.int32, device="cuda"), torch.zeros(samples, dtype=torch.int32, device="cuda")
        ch = chain.Chain(pus, fill, BD, clp, drec, avail, dluma, dorg, refs, pred, rec_a, lev_a)
        ch.gather()
        ch.repack()
        dpus, dfill = ops.struct_to_device(pus), ops.struct_to_device(fill)

        def entry():
            return ops.intra_chroma_code_batch(dorg, dpus, n, runs, rec_b, lev_b, None, (drec, avail, dfill), dluma, None, 0, BD, clp)

        def check(oc, oe):
            (sa, da), (sb, db) = oc, oe
            assert torch.equal(rec_a, rec_b) and torch.equal(lev_a, lev_b), name
            assert torch.equal(sa, sb.reshape(-1)) and torch.equal(da, db.reshape(-1)), name     # six slots in use: the items are the entry's, in its order
            return int((sb == 0).sum())

        kit.time_row("%-10s %6d %7d" % (name, n, 12 * n), ch.run, entry, check, WARMUP, RUNS)


if __name__ == "__main__":
    main()
