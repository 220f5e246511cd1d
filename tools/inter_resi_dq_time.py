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
depquant_listed_kernel (the trellis launch that the DepQuant entries share, depquant.hip) and inter_resi_dq_back_kernel.
The planes, build and the loop over the lists are the sibling's; the lists and the row come from tests/rd_pass_kit.py."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import inter_resi_code_time as sibling  # noqa: E402
import inter_resi_dq_cases as dqc  # noqa: E402
import inter_resi_dq_chain as chain  # noqa: E402
import rd_pass_kit as kit  # noqa: E402
from vvcsoftware_vtm_amd import abi  # noqa: E402

W, H, BD = sibling.W, sibling.H, sibling.BD
LAMBDA = 60.0
rng = np.random.default_rng(48)


def main():
    org, pred = sibling.planes(rng)
    cus = kit.timing_lists(rng, W, H, (8, 16, 32, 64))
    rates = dqc.shared_rates(8)

    def device_of(it, size):
        assert (it["level_off"] % 16 == 0).all()
        dq = np.zeros(len(it), abi.INTER_RESI_DQ)
        dq["lambda"], dq["rates_idx"], dq["luma"] = LAMBDA, np.arange(len(it)) % len(rates), np.arange(len(it)) % 3 == 0
        return chain.Device(BD, org, pred, it, dq, rates, size, size)

    sibling.time_lists(cus, device_of, chain.Chain, profile="--profile" in sys.argv)


if __name__ == "__main__":
    main()
