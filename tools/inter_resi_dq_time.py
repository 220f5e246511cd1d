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
--ts: the transform-skip candidate instead (VVCGPU_INTER_RESI_DQ_TS): at every CU position of the 4K list a 4x4 luma item, then a 4x4 Cb and a 4x4 Cr item,
each with the slots {DCT-II, transform skip} -- the blocks the reference tests the candidate on.  (a) is the same chain with tr_hor = 3 in the descriptors of
the skip slots (vvcgpu_tr_fwd_batch and vvcgpu_dequant_tr_inv_batch serve it), (b) the entry with the flag.
--profile: no timing, five runs of (b) per list -- the run to put under `rocprofv3 --kernel-trace --stats` for the split into inter_resi_dq_front_kernel,
depquant_listed_kernel (the trellis launch that the DepQuant entries share, depquant.hip) and inter_resi_dq_back_kernel.
The planes, build and the loop over the lists are the sibling's; the lists and the row come from tests/rd_pass_kit.py."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

import inter_resi_code_time as sibling  # noqa: E402
import inter_resi_dq_cases as dqc  # noqa: E402
import inter_resi_dq_chain as chain  # noqa: E402
import rd_pass_kit as kit  # noqa: E402
from vvcsoftware_vtm_amd import abi, ops  # noqa: E402

W, H, BD = sibling.W, sibling.H, sibling.BD
LAMBDA = 60.0
rng = np.random.default_rng(48)


def build_ts(px, py, chroma):
    """4x4 items with the slots {DCT-II, transform skip} at the CU positions: luma, or Cb and Cr (positions halved) -> the item records as the sibling's build"""
    comp = np.tile(np.arange(1, 3), len(px)) if chroma else np.zeros(len(px), np.int64)
    rep = 2 if chroma else 1
    s = (comp > 0).astype(np.int64)
    x, y = np.repeat(px, rep).astype(np.int64) >> s, np.repeat(py, rep).astype(np.int64) >> s
    it = np.zeros(len(comp), abi.INTER_RESI_ITEM)
    stride = np.where(comp == 0, W, W // 2)
    it["org_off"], it["org_stride"] = np.array([0, W * H, W * H + (W // 2) * (H // 2)])[comp] + y * stride + x, stride
    it["pred_off"], it["pred_stride"] = it["org_off"], stride
    it["cand_off"] = it["level_off"] = 32 * np.arange(len(comp))
    it["qp"], it["list_row"], it["w"], it["h"], it["sign_hiding"] = sibling.QP, -1, 4, 4, 1
    it["tr"] = -1
    it["tr"][:, 0], it["tr"][:, 1] = 0, abi.INTER_RESI_TS
    return it, 32 * len(comp)


class TsChain(chain.Chain):
    """the eight launches with the skip slots among the pairs: tr_hor = 3 in their descriptors of the forward and the inverse transform"""
    def __init__(self, D):
        items = D.items
        D.items = items.copy()
        D.items["tr"][items["tr"] == abi.INTER_RESI_TS] = 0                   # (the parent takes the slot for a DCT-II one: the same pairs and offsets)
        try:
            chain.Chain.__init__(self, D)
        finally:
            D.items = items
        pi, pk = self.pairs
        skip = items["tr"][pi, pk] == abi.INTER_RESI_TS
        area = items["w"].astype(np.int64) * items["h"]
        roff = np.concatenate([[0], np.cumsum(area)[:-1]])
        lev, cand = items["level_off"][pi] + pk * area[pi], items["cand_off"][pi] + pk * area[pi]
        code = np.where(skip, 0, items["tr"][pi, pk]).astype(np.int64)
        tr = np.zeros(self.m, abi.TR_DESC)
        tr["resi_off"], tr["coeff_off"], tr["resi_stride"], tr["w"], tr["h"] = roff[pi], lev, items["w"][pi], items["w"][pi], items["h"][pi]
        tr["tr_hor"], tr["tr_ver"] = np.where(skip, abi.TSKIP, code % 3), np.where(skip, 0, code // 3)
        dq = np.zeros(self.m, abi.DQTR_DESC)
        dq["resi_off"], dq["level_off"], dq["resi_stride"], dq["w"], dq["h"], dq["dep_quant"], dq["qp"] = cand, lev, items["w"][pi], items["w"][pi], items["h"][pi], 1, items["qp"][pi]
        dq["tr_hor"], dq["tr_ver"] = tr["tr_hor"], tr["tr_ver"]
        self.tr, self.dq = ops.struct_to_device(tr), ops.struct_to_device(dq)


def time_ts(cus, device_of, profile):
    """the 4K list's CU positions as 4x4 luma items, then as 4x4 chroma items: the chain and the entry with the flag compared, then timed, one row each"""
    _, _, _, px, py = cus[0]
    if not profile:
        print("list             items   slots   chain ms (min..max)   entry ms (min..max)   chain / entry   all-zero slots")
    for name, chroma in (("4K 4x4 luma", False), ("4K 4x4 chroma", True)):
        it, size = build_ts(px, py, chroma)
        D = device_of(it, size)
        rb, _, lb = D.fresh()

        def entry():
            return D.run_entry(rb, None, lb, abi.INTER_RESI_DQ_TS)

        if profile:
            for _ in range(5):
                entry()
            torch.cuda.synchronize()
            continue
        C = TsChain(D)
        ra, ca, la = D.fresh()

        def chained():
            return C.run(ra, ca, la)

        def check(oc, oe):
            assert C.same(oc, oe) and torch.equal(ra, rb) and torch.equal(la, lb), name
            return int((oc[0] == 0).sum())

        kit.time_row("%-14s %7d %7d" % (name + " +TS", len(it), C.m), chained, entry, check, sibling.WARMUP, sibling.RUNS)


def main():
    org, pred = sibling.planes(rng)
    cus = kit.timing_lists(rng, W, H, (8, 16, 32, 64))
    rates = dqc.shared_rates(8)

    def device_of(it, size):
        assert (it["level_off"] % 16 == 0).all()
        dq = np.zeros(len(it), abi.INTER_RESI_DQ)
        dq["lambda"], dq["rates_idx"], dq["luma"] = LAMBDA, np.arange(len(it)) % len(rates), np.arange(len(it)) % 3 == 0
        return chain.Device(BD, org, pred, it, dq, rates, size, size)

    if "--ts" in sys.argv:
        time_ts(cus, device_of, "--profile" in sys.argv)
        return
    sibling.time_lists(cus, device_of, chain.Chain, profile="--profile" in sys.argv)


if __name__ == "__main__":
    main()
