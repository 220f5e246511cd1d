#!/usr/bin/env python3
"""The inter residual pixel pass (InterSearch::encodeResAndCalcRdInterCU, InterSearch.cpp:4752-4909) of a 10-bit 3840x2160 4:2:0 picture, every CU as three
items (luma, Cb, Cr), every slot into candidate buffers of its own:
  4K      every interior 16x16 CU of the picture: a 16x16 luma item and two 8x8 chroma items;
  mix     8 000 CUs at random positions whose shapes follow the committed call trace (tests/golden/trace_ragop16_416x240_10b_q32.npz: the shapes of
          its pelop calls with sides 4..64), chroma halved;
each with one DCT-II slot per item, then once more with the four inter-EMT pairs as further slots of the luma items (sides 4..32).  The prediction is the
original moved by (1, -2) plus noise, QP 32, sign hiding on.
  (a) the chained form (tests/inter_resi_code_chain.py), built from entries whose code the new entry does not alter: pelop_batch subtract, tr_fwd_batch,
      quant_batch, dequant_tr_inv_batch, dist_batch twice, pelop_batch reco, dist_batch -- eight launches back to back, no host work between, descriptors
      uploaded outside the timed part;
  (b) vvcgpu_inter_resi_code_batch with WRITE_REC off: one launch.
The results of (a) and (b) are compared before anything is timed.  Times: device events around a whole run on the stream, 3 warm-up runs, then the median
and the spread of 9 runs, (a) and (b) alternating in one process.  The two lists and the row come from tests/rd_pass_kit.py."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import inter_resi_code_chain as chain  # noqa: E402
import pu_search_kit  # noqa: E402
import rd_pass_kit as kit  # noqa: E402
from vvcsoftware_vtm_amd import abi  # noqa: E402

W, H, BD = 3840, 2160, 10
QP = 32 + 12
EMT = (4, 5, 7, 8)
WARMUP, RUNS = 3, 9
rng = np.random.default_rng(47)


def build(w, h, px, py, emt):
    """CUs (luma w x h at (px, py)) -> the item records: per CU luma, Cb, Cr; contiguous predictions; six slots' room per item"""
    n = 3 * len(w)
    it = np.zeros(n, abi.INTER_RESI_ITEM)
    comp = np.tile(np.arange(3), len(w))
    s = (comp > 0).astype(np.int64)
    iw, ih = np.repeat(w, 3).astype(np.int64) >> s, np.repeat(h, 3).astype(np.int64) >> s
    x, y = np.repeat(px, 3).astype(np.int64) >> s, np.repeat(py, 3).astype(np.int64) >> s
    plane_off = np.array([0, W * H, W * H + (W // 2) * (H // 2)])[comp]
    stride = np.where(comp == 0, W, W // 2)
    area = iw * ih
    slots = np.where(emt & (comp == 0) & (iw <= 32) & (ih <= 32), 5, 1)
    it["org_off"], it["org_stride"] = plane_off + y * stride + x, stride
    it["pred_off"], it["pred_stride"] = it["org_off"], stride                # the prediction planes have the original's layout
    room = np.concatenate([[0], np.cumsum(slots * area)[:-1]])
    it["cand_off"], it["level_off"] = room, room
    it["qp"], it["list_row"], it["w"], it["h"], it["sign_hiding"] = QP, -1, iw, ih, 1
    it["tr"] = -1
    it["tr"][:, 0] = 0
    for k, c in enumerate(EMT):
        it["tr"][slots == 5, 1 + k] = c
    return it, int((slots * area).sum())


def planes(rng):
    """-> (org, pred): the three planes of the picture one after another; the prediction is the original moved by (1, -2) plus noise"""
    luma = pu_search_kit.texture(rng, H, W, BD, 0.0)
    yuv = [luma, np.ascontiguousarray(luma[0::2, 0::2]), np.ascontiguousarray(luma[1::2, 1::2])]
    org = np.concatenate([p.reshape(-1) for p in yuv])
    pred = np.concatenate([np.clip(np.roll(p, (1, -2), axis=(0, 1)).astype(np.int32) + rng.integers(-4, 5, p.shape), 0, 1023).astype(np.int16).reshape(-1) for p in yuv])
    return org, pred


def time_lists(cus, device_of, chain_of, profile=False):
    """every list without and with the EMT slots: the chain and the entry compared, then timed, one row each (profile: five runs of the entry instead)"""
    if not profile:
        print("list             items   slots   chain ms (min..max)   entry ms (min..max)   chain / entry   all-zero slots")
    for emt in (False, True):
        for name, w, h, px, py in cus:
            it, size = build(w, h, px, py, emt)
            D = device_of(it, size)
            rb, _, lb = D.fresh()

            def entry():
                return D.run_entry(rb, None, lb, 0)

            if profile:
                for _ in range(5):
                    entry()
                torch.cuda.synchronize()
                continue
            C = chain_of(D)
            ra, ca, la = D.fresh()

            def chained():
                return C.run(ra, ca, la)

            def check(oc, oe):
                assert C.same(oc, oe) and torch.equal(ra, rb) and torch.equal(la, lb), name
                return int((oc[0] == 0).sum())

            kit.time_row("%-14s %7d %7d" % (name + (" +EMT" if emt else ""), len(it), C.m), chained, entry, check, WARMUP, RUNS)


def main():
    org, pred = planes(rng)
    cus = kit.timing_lists(rng, W, H, (4, 8, 16, 32, 64))
    time_lists(cus, lambda it, size: chain.Device(BD, org, pred, it, size, size), chain.Chain)


if __name__ == "__main__":
    main()
