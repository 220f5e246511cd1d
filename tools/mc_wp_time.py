"""Times vvcgpu_mc_picture_batch against vvcgpu_mc_wp_batch on the PU list of the 4K workload (Workload(3840, 2160).mc_pic: 16x16 luma, 8x8 chroma,
uni and bi): unweighted, weighted with default weights, weighted bi with non-trivial weights, and every PU weighted uni.  Prints us per picture from
events over repeated calls, one JSON line.  Usage: python tools/mc_wp_time.py [--reps 200]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from vvcsoftware_vtm_amd import ops  # noqa: E402
from vvcsoftware_vtm_amd.workload import Workload  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    a = ap.parse_args()
    wl = Workload(3840, 2160, 10)
    st, _ = wl.run_gpu(None, None)
    torch.cuda.synchronize()
    bd, mx, n = 10, 1023, wl.mc_pic.size
    d = wl.mc_pic
    ref0, ref1, pred = st["ref0"][0], st["ref1"][0], st["pred"][0]

    def wp_list(descs, records, uni_all=False):
        q = descs.copy()
        if uni_all:
            q["bi"] = 0
        q["reserved"] = np.where(q["bi"] == 1, 1, 0)
        return ops.struct_to_device(q), ops.struct_to_device(np.array(records, dtype=ops.WP_PARAM))

    forms = {"picture_batch": None,
             "wp_default": wp_list(d, [ops.wp_param(bd, 6, 64, 0), ops.wp_param(bd, 6, 64, 0, 64, 0)]),
             "wp_bi_weighted": wp_list(d, [ops.wp_param(bd, 6, 45, -3), ops.wp_param(bd, 6, 45, -3, 83, 7)]),
             "wp_uni_weighted": wp_list(d, [ops.wp_param(bd, 6, 45, -3), ops.wp_param(bd, 6, 45, -3, 83, 7)], uni_all=True)}
    out = {"n_pus": int(n), "bi_fraction": float((d["bi"] == 1).mean())}
    for name, f in forms.items():
        if f is None:
            fn = lambda: ops.mc_picture_batch(ref0, ref1, pred, st["mc_pic"], n, bd, (0, mx))
        else:
            fn = lambda f=f: ops.mc_wp_batch(ref0, ref1, pred, f[0], n, f[1], 2, bd, (0, mx))
        for _ in range(10):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out[name + "_us"] = round(e0.elapsed_time(e1) / a.reps * 1e3, 2)
    out["wp_bi_weighted_vs_picture_batch"] = round(out["wp_bi_weighted_us"] / out["picture_batch_us"], 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
