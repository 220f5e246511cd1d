#!/usr/bin/env python3
"""Whole bi-predictive refinements (the loop of InterSearch::predInterSearch, InterSearch.cpp:1058-1164), two lists:
  4K      every 16x16 PU of a 3840x2160 10-bit picture (32 400 PUs);
  mix     about 8 000 PUs at random positions of the same picture whose shapes follow the bi-predicted blocks of the committed call trace
          (tests/golden/trace_ragop16_416x240_10b_q32.npz: the addAvg calls, sides 4..128, powers of two -- the trace records no removeHighFreq call).
Two reference pictures per list out of four planes; originals = the mean of the planes plus noise, entries displaced, so the refinements move.
  (a) the chained form (tests/bipred_me_chain.py), built from entries the library already had: per iteration vvcgpu_mc_batch -> vvcgpu_pelop_batch ->
      per reference index vvcgpu_sad_search per (shape, plane), download of the SAD surfaces, vector costs and arg-min on the host,
      vvcgpu_frac_refine, download, cost and keep-if-better on the host (vectorised numpy);
  (b) vvcgpu_bipred_me_batch: upload of the items, one call, download of the results.
The results of (a) and (b) are compared before anything is timed.  Times: device events around a whole run on the stream (for (a) that includes the
device's idle time while the host decides: it is what the caller waits for), 3 warm-up runs, then the median and the spread of 7 runs, (a) and (b)
alternating.  The device time of (b)'s launch alone is given too."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bipred_me_cases as bc  # noqa: E402
import pu_search_kit as kit  # noqa: E402
import bipred_me_chain  # noqa: E402
from vvcsoftware_vtm_amd import abi, ops, shape_mix  # noqa: E402

W, H, BD, M = 3840, 2160, 10, bc.MARGIN
LAMBDA, N_PLANES, N_REF = 37.5, 4, (2, 2)
PRED = (4, -8)                               # the one vector predictor of every item (what the public entries of the chain can take per call)
WARMUP, RUNS = 3, 7
rng = np.random.default_rng(23)


def build_items(shapes, pos):
    items = np.zeros(len(shapes), abi.BIPRED_ME_ITEM)
    for i, ((w, h), (px, py)) in enumerate(zip(shapes, pos)):
        base = rng.integers(-24, 25, 2)
        refs = [[bc.ref_record(int(rng.integers(0, N_PLANES)), list(base + rng.integers(-10, 11, 2)), [list(PRED)], 0) for _ in range(N_REF[l])] for l in range(2)]
        sad = w * h * 12
        items[i] = bc.item(px, py, w, h, 0, py * W + px, W, refs, [int(rng.integers(0, N_REF[0])), int(rng.integers(0, N_REF[1]))],
                           [int(sad * rng.uniform(0.6, 1.6)), int(sad * rng.uniform(0.6, 1.6))], [int(rng.integers(8, 30)), int(rng.integers(8, 30))])
    return items


def main():
    planes = np.stack([kit.texture(rng, H, W, BD, 1.5 * k) for k in range(N_PLANES)])
    org = np.clip(planes.astype(np.int32).mean(axis=0) + rng.integers(-6, 7, (H, W)), 0, 1023).astype(np.int16)
    d_org, d_planes = torch.from_numpy(org).cuda(), torch.from_numpy(kit.pad(planes)).cuda()
    cfg = bc.cfg_dict(LAMBDA, W, H, BD, mvp_idx_cost=(1, 1, 0))
    hist, _ = shape_mix.load_trace()
    sig = shape_mix.signatures(hist, "pelop", lambda w, h, a, b, c: a == 0 and w in bc.SIDES and h in bc.SIDES)
    mix = [(int(w), int(h)) for w, h in sig[rng.choice(len(sig), 8000, p=sig[:, 5] / sig[:, 5].sum()), :2]]
    lists = [("4K 16x16", [(16, 16)] * ((W // 16) * (H // 16)), [(x, y) for y in range(0, H, 16) for x in range(0, W, 16)], (16, 16)),
             ("trace mix", mix, [(int(rng.integers(0, (W - w) // 4 + 1)) * 4, int(rng.integers(0, (H - h) // 4 + 1)) * 4) for w, h in mix], (0, 0))]
    print("list          PUs   ME calls  chain launches   chain ms (min..max)     one launch ms (min..max)   kernel ms   chain / one launch")
    for name, shapes, pos, max_pu in lists:
        items = build_items(shapes, pos)
        n = len(items)
        m = bc.MARGIN
        dcfg = ops.bipred_me_cfg(LAMBDA, [d_planes[i] for i in range(N_PLANES)], (m, m), W, H, BD, (0, 1023), 4, False, False, 4, True, True, (1, 1, 0), 128, max_pu)

        def one_call():
            d_items = ops.struct_to_device(items)
            r, _ = ops.bipred_me_batch(d_org, d_items, n, dcfg, want_trace=False)
            return r.cpu().numpy().view(abi.BIPRED_ME_RESULT)

        def chain():
            return bipred_me_chain.chained(d_org, d_planes, cfg, items, m)

        res = one_call()
        got, launches = chain()
        for f in ("mv", "ref_idx", "bits", "mot_bits", "me_calls", "closing", "cost"):
            assert np.array_equal(got[f], res[f]), (name, f)
        ta, tb = kit.times_of_alternating((chain, one_call), WARMUP - 1, RUNS)              # the comparison above was the first warm-up run
        d_items = ops.struct_to_device(items)
        tk = sorted(kit.events(lambda: ops.bipred_me_batch(d_org, d_items, n, dcfg, want_trace=False))[0] for _ in range(RUNS))[RUNS // 2]
        a, b = float(np.median(ta)), float(np.median(tb))
        print("%-10s %6d  %9d  %14d   %8.2f (%.2f..%.2f)   %8.2f (%.2f..%.2f)   %9.2f   %8.2f" %
              (name, n, int(res["me_calls"].sum()), launches, a, min(ta), max(ta), b, min(tb), max(tb), tk, a / b))


if __name__ == "__main__":
    main()
