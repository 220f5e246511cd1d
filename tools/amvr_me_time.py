#!/usr/bin/env python3
"""The AMVR passes (cu.imv = 1, 2: integer-sample and four-sample vectors) of the translational inter search of a PU, two references per list, once per imv:
  4K      every 16x16 PU of a 3840x2160 10-bit picture (32 400 PUs, 129 600 searches), max_pu 16x16;
  mix     about 8 000 PUs at random positions of the same picture whose shapes follow the committed call trace
          (tests/golden/trace_ragop16_416x240_10b_q32.npz: the shapes of its pelop calls, sides 4..128, powers of two).
The inputs are tools/unipred_me_time.py's, the candidates rounded to the pass's resolution as PU::fillMvpCand rounds them.
  (a) the chained form (tests/amvr_me_chain.py), built from entries that do not know cfg.imv: one vvcgpu_mc_dist_batch, download, predictor choice on
      the host, one vvcgpu_tz_search_batch with imv_shift per (list, reference) and owner kind, download, one vvcgpu_imv_refine_batch per (list, reference), download,
      keep-if-better on the host (vectorised numpy);
  (b) vvcgpu_unipred_me_batch with cfg.imv: upload of the items, one call, download of the results;
  (c) (b) without the download, followed by vvcgpu_bipred_me_batch with cfg.imv on the first call's out-items, download of the bi-predictive results.
The results of (a) and (b) are compared before anything is timed.  Times: device events around a whole run on the stream (for (a) that includes the
device's idle time while the host decides: it is what the caller waits for), 3 warm-up runs, then the median and the spread of 7 runs, (a), (b) and (c)
alternating.  The device time of (b)'s two launches alone is given too."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import unipred_me_cases as uc  # noqa: E402
import pu_search_kit as kit  # noqa: E402
import amvr_me_cases as am  # noqa: E402
import amvr_me_chain  # noqa: E402
from vvcsoftware_vtm_amd import abi, ops, shape_mix  # noqa: E402

W, H, BD, M = 3840, 2160, 10, uc.MARGIN
LAMBDA, N_PLANES, N_REF, RANGE = 37.5, 4, (2, 2), 32
WARMUP, RUNS = 3, 7
rng = np.random.default_rng(29)


def build_items(shapes, pos):
    n = len(shapes)
    items = np.zeros(n, abi.UNIPRED_ME_ITEM)
    wh, xy = np.array(shapes), np.array(pos)
    items["w"], items["h"], items["pos_x"], items["pos_y"] = wh[:, 0], wh[:, 1], xy[:, 0], xy[:, 1]
    items["sub_shift"] = (wh[:, 1] > 8) & (wh[:, 0] <= 64)
    items["org_off"], items["org_stride"] = xy[:, 1].astype(np.int64) * W + xy[:, 0], W
    items["mb_bits"] = rng.integers(1, 6, (n, 3))
    base = np.array([20, -12]) + rng.integers(-24, 25, (n, 2, 4, 1, 2))
    cand = base + rng.integers(-9, 10, (n, 2, 4, 2, 2))
    num = rng.integers(1, 3, (n, 2, 4))
    cand[..., 1, :] = np.where((num == 1)[..., None], cand[..., 0, :], cand[..., 1, :])
    items["ref"]["mv_cand"], items["ref"]["num_cand"] = cand, num
    items["ref"]["flags"] = rng.integers(0, 2, (n, 2, 4)) * abi.UNIPRED_PRED2
    items["ref"]["pred2"] = rng.integers(-12, 13, (n, 2, 4, 2))
    return items


def main():
    planes = np.stack([kit.texture(rng, H, W, BD, 1.5 * k) for k in range(N_PLANES)])
    org = np.clip(np.roll(planes[0], (3, -5), axis=(0, 1)).astype(np.int32) + rng.integers(-6, 7, (H, W)), 0, 1023).astype(np.int16)
    d_org, d_planes = torch.from_numpy(org).cuda(), torch.from_numpy(kit.pad(planes)).cuda()
    cfg = uc.cfg_dict(LAMBDA, W, H, BD, n_ref=N_REF, search_range=RANGE)
    hist, _ = shape_mix.load_trace()
    sig = shape_mix.signatures(hist, "pelop", lambda w, h, a, b, c: a == 0 and w in uc.SIDES and h in uc.SIDES)
    mix = [(int(w), int(h)) for w, h in sig[rng.choice(len(sig), 8000, p=sig[:, 5] / sig[:, 5].sum()), :2]]
    lists = [("4K 16x16", [(16, 16)] * ((W // 16) * (H // 16)), [(x, y) for y in range(0, H, 16) for x in range(0, W, 16)], (16, 16)),
             ("trace mix", mix, [(int(rng.integers(0, (W - w) // 4 + 1)) * 4, int(rng.integers(0, (H - h) // 4 + 1)) * 4) for w, h in mix], (0, 0))]
    print("list       imv     PUs  shapes  chain calls   chain ms (min..max)   of it host ms   entry ms (min..max)   launches ms   entry + bipred ms (min..max)   chain / entry")
    for name, shapes, pos, max_pu, imv in [l + (imv,) for l in lists for imv in (1, 2)]:
        items = am.align_items(build_items(shapes, pos), imv)
        n = len(items)
        planes_l = [d_planes[i] for i in range(N_PLANES)]
        dcfg = ops.unipred_me_cfg(LAMBDA, planes_l, (M, M), W, H, N_REF, cfg["ref_plane"], cfg["search_range"], BD, (0, 1023), max_pu=max_pu, imv=imv)
        dbcfg = ops.bipred_me_cfg(LAMBDA, planes_l, (M, M), W, H, BD, (0, 1023), 4, False, False, 4, True, True, (1, 1, 0), 128, max_pu, imv=imv)
        host = []

        def entry():
            r, _ = ops.unipred_me_batch(d_org, ops.struct_to_device(items), n, dcfg, want_bipred_items=False)
            return r.cpu().numpy().view(abi.UNIPRED_ME_RESULT)

        def entry_bipred():
            _, out = ops.unipred_me_batch(d_org, ops.struct_to_device(items), n, dcfg)
            r, _ = ops.bipred_me_batch(d_org, out, n, dbcfg, want_trace=False)
            return r.cpu().numpy().view(abi.BIPRED_ME_RESULT)

        def chain():
            ch = amvr_me_chain.Chain(d_org, d_planes, cfg, items, M, imv)
            r = ch.run()
            host.append(ch.host_s * 1e3)
            return r, ch.launches

        res = entry()
        got, calls = chain()
        for f in res.dtype.names:
            assert np.array_equal(got[f], res[f]), (name, imv, f)
        bi = entry_bipred()
        assert (bi["cost"] != np.uint64(kit.U64_MAX)).all()
        ta, tb, tc = kit.times_of_alternating((chain, entry, entry_bipred), WARMUP - 1, RUNS)   # the comparison above was the first warm-up run
        d_items = ops.struct_to_device(items)
        tk = sorted(kit.events(lambda: ops.unipred_me_batch(d_org, d_items, n, dcfg, want_bipred_items=False))[0] for _ in range(RUNS))[RUNS // 2]
        a, b, c = float(np.median(ta)), float(np.median(tb)), float(np.median(tc))
        print("%-10s %3d  %6d  %6d  %11d   %8.2f (%.2f..%.2f)   %10.2f   %8.2f (%.2f..%.2f)   %11.2f   %8.2f (%.2f..%.2f)   %10.2f" %
              (name, imv, n, len(set(shapes)), calls, a, min(ta), max(ta), float(np.median(host[-RUNS:])), b, min(tb), max(tb), tk, c, min(tc), max(tc), a / b))


if __name__ == "__main__":
    main()
