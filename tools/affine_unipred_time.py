#!/usr/bin/env python3
"""Whole affine uni-predictive stages (the uni-predictive part of InterSearch::xPredAffineInterSearch, InterSearch.cpp:2651-2814), two lists:
  16x16   every 16x16 PU of a 3840x2160 10-bit picture (32 400 PUs, max_pu 16x16: wavefront owners);
  64x64   every 64x64 PU of the same picture (1 980 PUs, max_pu 64x64: workgroup owners).
4- and 6-parameter PUs alternate; two reference pictures per list, four planes in all (list 0: planes 0 and 1, list 1: planes 2 and 3); the original is
the first plane plus noise, the candidates, the translational vector and the 4-parameter vectors are displaced from a common motion, so the searches move.
  (a) the chained form (tests/affine_unipred_chain.py), built from entries the library already had: vvcgpu_affine_pred_batch per plane and
      vvcgpu_dist_batch for the template costs, download, the predictor and start choice on the host (vectorised numpy), upload,
      vvcgpu_affine_me_batch per plane, download, the shortcut, xCheckBestAffineMVP and the records on the host;
  (b) vvcgpu_affine_unipred_me_batch: upload of the items, one call (two launches), download of the results;
  (c) as (b), then vvcgpu_affine_bipred_me_batch on the out-items as they lie in device memory, download of both results.
The results of (a) and (b) are compared before anything is timed.  Times: device events around a whole run on the stream (for (a) that includes the
device's idle time while the host decides: it is what the caller waits for), 3 warm-up runs, then the median and the spread of 7 runs, the forms
alternating.  The device time of (b)'s two launches alone is given too, and the kernels' resource lines where the built object is at hand."""
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import affine_unipred_cases as uc  # noqa: E402
import pu_search_kit as kit  # noqa: E402
import affine_unipred_chain  # noqa: E402
from vvcsoftware_vtm_amd import abi, ops  # noqa: E402

W, H, BD, M = 3840, 2160, 10, uc.MARGIN
LAMBDA, N_PLANES, N_REF = 37.5, 4, (2, 2)
REF_PLANE = ((0, 1, 0, 1), (2, 3, 2, 3))        # plane of (list, reference index): every plane is some list's reference
WARMUP, RUNS = 3, 7
rng = np.random.default_rng(31)


def build_items(side):
    """every side x side PU of the picture, vectorised: per (list, reference) two candidates, the translational vector and the 4-parameter vectors around
    a common motion; a 6-parameter PU carries only_ref >= 0 for both lists"""
    xs, ys = np.meshgrid(np.arange(0, W - side + 1, side), np.arange(0, H - side + 1, side))
    px, py = xs.reshape(-1), ys.reshape(-1)
    n = len(px)
    items = np.zeros(n, abi.AFFINE_UNIPRED_ITEM)
    items["pos_x"], items["pos_y"], items["w"], items["h"], items["six_param"] = px, py, side, side, np.arange(n) & 1
    items["org_off"], items["org_stride"], items["mb_bits"] = py.astype(np.int64) * W + px, W, (2, 2, 4)
    base = rng.integers(-10, 11, (n, 1, 1, 1, 2)) * 4
    rec = items["ref"]
    rec["mv_cand"] = base[:, :, :, None] + rng.integers(-3, 4, (n, 2, 4, 2, 3, 2)) * 4
    rec["hevc_mv"] = base[:, :, :, 0] + rng.integers(-3, 4, (n, 2, 4, 2)) * 4
    rec["mv4"] = base + rng.integers(-3, 4, (n, 2, 4, 2, 2)) * 4
    rec["num_cand"] = 2
    items["ref"] = rec
    ri = np.stack([rng.integers(0, N_REF[0], n), rng.integers(0, N_REF[1], n)], axis=1)
    items["only_ref"] = np.where((items["six_param"] != 0)[:, None], ri, -1)
    return items


def main():
    planes, org = kit.planes_and_first_org(rng, N_PLANES, W, H, BD)
    d_org, d_planes = torch.from_numpy(org).cuda(), torch.from_numpy(kit.pad(planes)).cuda()
    cfg = uc.cfg_dict(LAMBDA, W, H, BD, n_ref=N_REF, ref_plane=REF_PLANE)
    pl = [d_planes[i] for i in range(N_PLANES)]
    print("list       PUs  searches  (a) launches   (a) chain ms (min..max)    (b) entry ms (min..max)   (b) kernels ms   (c) entry + bi ms (min..max)   (a) / (b)")
    for side in (16, 64):
        items = build_items(side)
        n = len(items)
        dcfg = ops.affine_unipred_cfg(LAMBDA, pl, (M, M), W, H, N_REF, cfg["ref_plane"], BD, (0, 1023), cfg["list1_to_list0"], False, False, 1, (1, 1, 0), 128,
                                      (side, side))
        dbcfg = ops.affine_bipred_cfg(LAMBDA, pl, (M, M), W, H, BD, (0, 1023), 4, False, False, True, 1, (1, 1, 0), 128, (side, side))

        def entry():
            d_items = ops.struct_to_device(items)
            r, _ = ops.affine_unipred_me_batch(d_org, d_items, n, dcfg, want_bipred_items=False)
            return r.cpu().numpy().view(abi.AFFINE_UNIPRED_RESULT)

        def entry_bi():
            d_items = ops.struct_to_device(items)
            r, out = ops.affine_unipred_me_batch(d_org, d_items, n, dcfg)
            bi, _ = ops.affine_bipred_me_batch(d_org, out, n, dbcfg, want_trace=False)
            return r.cpu().numpy().view(abi.AFFINE_UNIPRED_RESULT), bi.cpu().numpy().view(abi.AFFINE_BIPRED_RESULT)

        def chain():
            return affine_unipred_chain.chained(d_org, d_planes, cfg, items, M)

        res = entry()
        got, launches = chain()
        for f in res.dtype.names:
            assert np.array_equal(got[f], res[f]), (side, f)
        r2, bi = entry_bi()
        assert np.array_equal(r2, res) and (bi["cost"] != np.uint64(kit.U64_MAX)).all()
        ta, tb, tc = kit.times_of_alternating((chain, entry, entry_bi), WARMUP - 1, RUNS)   # the comparison above was the first warm-up run
        d_items = ops.struct_to_device(items)
        tk = sorted(kit.events(lambda: ops.affine_unipred_me_batch(d_org, d_items, n, dcfg, want_bipred_items=False))[0] for _ in range(RUNS))[RUNS // 2]
        a, b, c = float(np.median(ta)), float(np.median(tb)), float(np.median(tc))
        print("%-7s %6d  %8d  %12d   %9.2f (%.2f..%.2f)   %9.2f (%.2f..%.2f)   %14.2f   %9.2f (%.2f..%.2f)   %9.2f" %
              ("%dx%d" % (side, side), n, int((res["s"]["searched"] == 1).sum()), launches, a, min(ta), max(ta), b, min(tb), max(tb), tk, c, min(tc), max(tc), a / b),
              flush=True)
    obj = os.path.join(ROOT, "vvcsoftware_vtm_amd", "lib", "obj", "affine_unipredme.o")
    if os.path.exists(obj):
        print(subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "affine_unipredme"], capture_output=True, text=True).stdout)


if __name__ == "__main__":
    main()
