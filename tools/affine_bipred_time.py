#!/usr/bin/env python3
"""Whole affine bi-predictive searches (the bi-predictive part of InterSearch::xPredAffineInterSearch, InterSearch.cpp:2823-2997), two lists:
  16x16   every 16x16 PU of a 3840x2160 10-bit picture (32 400 PUs, max_pu 16x16: wavefront owners);
  64x64   every 64x64 PU of the same picture (1 980 PUs, max_pu 64x64: workgroup owners).
4- and 6-parameter PUs alternate; two reference pictures per list out of four planes; originals = the mean of the planes plus noise, entry vectors
displaced, so the searches move.
  (a) the chained form (tests/affine_bipred_chain.py), built from entries the library already had: per iteration vvcgpu_affine_pred_batch per plane ->
      vvcgpu_pelop_batch -> per reference index vvcgpu_affine_me_batch per plane, download, xCheckBestAffineMVP and keep-if-better on the host
      (vectorised numpy), upload;
  (b) vvcgpu_affine_bipred_me_batch: upload of the items, one call, download of the results.
The results of (a) and (b) are compared before anything is timed.  Times: device events around a whole run on the stream (for (a) that includes the
device's idle time while the host decides: it is what the caller waits for), 3 warm-up runs, then the median and the spread of 7 runs, (a) and (b)
alternating.  The device time of (b)'s launch alone is given too, and the kernel's resource line where the built object is at hand."""
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import affine_bipred_cases as ac  # noqa: E402
import pu_search_kit as kit  # noqa: E402
import affine_bipred_chain  # noqa: E402
from vvcsoftware_vtm_amd import abi, ops  # noqa: E402

W, H, BD, M = 3840, 2160, 10, ac.MARGIN
LAMBDA, N_PLANES, N_REF = 37.5, 4, (2, 2)
WARMUP, RUNS = 3, 7
rng = np.random.default_rng(29)


def build_items(side):
    """every side x side PU of the picture, vectorised: control points around a common translation, two candidates per (list, reference)"""
    xs, ys = np.meshgrid(np.arange(0, W - side + 1, side), np.arange(0, H - side + 1, side))
    px, py = xs.reshape(-1), ys.reshape(-1)
    n = len(px)
    items = np.zeros(n, abi.AFFINE_BIPRED_ITEM)
    items["pos_x"], items["pos_y"], items["w"], items["h"], items["six_param"] = px, py, side, side, np.arange(n) & 1
    items["org_off"], items["org_stride"], items["n_ref"] = py.astype(np.int64) * W + px, W, N_REF
    base = rng.integers(-10, 11, (n, 1, 1, 1, 2)) * 4
    rec = items["ref"]
    rec["plane"] = rng.integers(0, N_PLANES, (n, 2, 4))
    rec["mv"] = base + rng.integers(-6, 7, (n, 2, 4, 3, 2)) * 4
    rec["mv_cand"] = base[:, :, :, None] + rng.integers(-3, 4, (n, 2, 4, 2, 3, 2)) * 4
    rec["num_cand"], rec["mvp_idx"] = 2, rng.integers(0, 2, (n, 2, 4))
    items["ref"] = rec
    ri = np.stack([rng.integers(0, N_REF[0], n), rng.integers(0, N_REF[1], n)], axis=1)
    items["ref_idx"] = ri
    items["only_ref"] = np.where((items["six_param"] != 0)[:, None], ri, -1)
    for l in range(2):
        items["mv"][:, l] = items["ref"]["mv"][np.arange(n), l, ri[:, l]]
    had = side * side * 12
    items["cost"] = (had * rng.uniform(0.5, 1.4, (n, 2))).astype(np.uint64)
    items["bits"], items["mb_bits"] = rng.integers(8, 30, (n, 2)), (2, 2, 4)
    return items


def main():
    planes, org = kit.planes_and_mean_org(rng, N_PLANES, W, H, BD)
    d_org, d_planes = torch.from_numpy(org).cuda(), torch.from_numpy(kit.pad(planes)).cuda()
    cfg = ac.cfg_dict(LAMBDA, W, H, BD, mvp_idx_cost=(1, 1, 0))
    print("list       PUs   ME calls  chain launches   chain ms (min..max)     one launch ms (min..max)   kernel ms   chain / one launch")
    for side in (16, 64):
        items = build_items(side)
        n = len(items)
        dcfg = ops.affine_bipred_cfg(LAMBDA, [d_planes[i] for i in range(N_PLANES)], (M, M), W, H, BD, (0, 1023), 4, False, False, True, 1, (1, 1, 0), 128, (side, side))

        def one_call():
            d_items = ops.struct_to_device(items)
            r, _ = ops.affine_bipred_me_batch(d_org, d_items, n, dcfg, want_trace=False)
            return r.cpu().numpy().view(abi.AFFINE_BIPRED_RESULT)

        def chain():
            return affine_bipred_chain.chained(d_org, d_planes, cfg, items, M)

        res = one_call()
        got, launches = chain()
        for f in ("mv", "ref_idx", "mvp_idx", "mvp", "bits", "mot_bits", "me_calls", "closing", "cost"):
            assert np.array_equal(got[f], res[f]), (side, f)
        ta, tb = kit.times_of_alternating((chain, one_call), WARMUP - 1, RUNS)              # the comparison above was the first warm-up run
        d_items = ops.struct_to_device(items)
        tk = sorted(kit.events(lambda: ops.affine_bipred_me_batch(d_org, d_items, n, dcfg, want_trace=False))[0] for _ in range(RUNS))[RUNS // 2]
        a, b = float(np.median(ta)), float(np.median(tb))
        print("%-7s %6d  %9d  %14d   %8.2f (%.2f..%.2f)   %8.2f (%.2f..%.2f)   %9.2f   %8.2f" %
              ("%dx%d" % (side, side), n, int(res["me_calls"].sum()), launches, a, min(ta), max(ta), b, min(tb), max(tb), tk, a / b), flush=True)
    obj = os.path.join(ROOT, "vvcsoftware_vtm_amd", "lib", "obj", "affine_bipredme.o")
    if os.path.exists(obj):
        print(subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "affine_bipredme"], capture_output=True, text=True).stdout)


if __name__ == "__main__":
    main()
