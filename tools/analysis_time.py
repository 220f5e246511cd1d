"""Times the encoder picture analysis entries on the 4K bench picture (Workload(3840, 2160).org) and on 1920x1080: event-timed microseconds per call
(calls queued back to back on one stream) over input sets that rotate as the bench rotates its inputs (12 sets: a 4K set is 50 MB with its
reconstruction, so no call finds its planes in the 256 MiB last-level cache), beside the bytes each entry reads, that count over the project's 8 TB/s figure, and the download of the picture the
entry replaces (43 GB/s).  Prints one table and one JSON line.  Usage: python tools/analysis_time.py [--reps 120] [--sets 12]"""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from vvcsoftware_vtm_amd import capi, ops  # noqa: E402
from vvcsoftware_vtm_amd.workload import Workload  # noqa: E402

HBM_BPS, DOWNLOAD_BPS = 8e12, 43e9


def timed(fn, reps, sets):
    for i in range(2 * sets):
        fn(i % sets)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(reps):
        fn(i % sets)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=120)
    ap.add_argument("--sets", type=int, default=12)
    a = ap.parse_args()
    bd = 10
    cands = ops.wp_sad_cands([(6, 64, 0, 0), (6, 64, 0, 2), (6, 58, 3, 0), (6, 58, 3, 2), (6, 70, -4, 0), (6, 70, -4, 2), (7, 120, 2, 1), (7, 120, 2, 3),
                              (5, 30, 1, 0), (5, 30, 1, 2), (5, 34, -1, 0), (5, 34, -1, 2), (6, 61, 5, 1), (6, 61, 5, 3), (6, 67, -6, 1), (6, 67, -6, 3)])
    report = {}
    for (w, h, tile) in ((3840, 2160, 128), (1920, 1080, 64)):
        wl = Workload(w, h, bd)
        rng = np.random.default_rng(1)
        sets = []
        for k in range(a.sets):
            org = [np.roll(p, 8 * k, axis=1) for p in wl.org]                   # every set its own memory and its own content
            rec = [np.clip(p.astype(np.int32) + rng.integers(-4, 5, p.shape), 0, (1 << bd) - 1).astype(np.int16) for p in org]
            sets.append(([torch.from_numpy(np.ascontiguousarray(p)).cuda() for p in org], [torch.from_numpy(p).cuda() for p in rec]))
        pic = sum(int(p.size) for p in wl.org) * 2
        luma = int(wl.org[0].size) * 2
        # the C entries with prepared arguments and outputs (what a binding does), so that the host's share of a call is ctypes and two launches only
        po, pr = [ops.planes(s_[0]) for s_ in sets], [ops.planes(s_[1]) for s_ in sets]
        ntile = [(-(-(h >> (c > 0)) // (tile >> (c > 0)))) * (-(-(w >> (c > 0)) // (tile >> (c > 0)))) for c in range(3)]
        o_tile = [torch.empty((n, 3), dtype=torch.int64, device="cuda") for n in ntile]
        o_sse, o_hist = torch.empty(3, dtype=torch.int64, device="cuda"), torch.empty((3, 1 << bd), dtype=torch.int32, device="cuda")
        o_sad, o_cost = torch.empty(16, dtype=torch.int64, device="cuda"), torch.empty(-(-h // 128) * -(-w // 128), dtype=torch.int32, device="cuda")
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        cp = cands.ctypes.data_as(C.c_void_p)
        t3 = [capi.ptr(t) for t in o_tile]
        yo, yr = [capi.ptr(s_[0][0]) for s_ in sets], [capi.ptr(s_[1][0]) for s_ in sets]
        call = capi.call
        entries = [
            ("tile_stats_picture (org + rec, tile %d)" % tile, 2 * pic,
             lambda i: call("vvcgpu_tile_stats_picture", C.byref(po[i]), C.byref(pr[i]), w, h, tile, 3, t3[0], t3[1], t3[2], st)),
            ("tile_stats_picture (rec null, tile %d)" % tile, pic,
             lambda i: call("vvcgpu_tile_stats_picture", C.byref(po[i]), None, w, h, tile, 3, t3[0], t3[1], t3[2], st)),
            ("picture_sse", 2 * pic, lambda i: call("vvcgpu_picture_sse", C.byref(po[i]), C.byref(pr[i]), w, h, 3, capi.ptr(o_sse), st)),
            ("picture_histogram", pic, lambda i: call("vvcgpu_picture_histogram", C.byref(po[i]), w, h, 3, bd, capi.ptr(o_hist), st)),
        ] + [("wp_sad_batch (luma, %d candidate%s)" % (n, "s" if n > 1 else ""), 2 * luma,
              lambda i, n=n: call("vvcgpu_wp_sad_batch", yo[i], w, yr[i], w, w, h, bd, cp, n, capi.ptr(o_sad), st)) for n in (16, 4, 1)] + [
            ("intra_cost_ctus (luma, CTU 128)", luma, lambda i: call("vvcgpu_intra_cost_ctus", yo[i], w, w, h, 128, bd, capi.ptr(o_cost), st)),
        ]
        download_us = pic / DOWNLOAD_BPS * 1e6
        print("%dx%d %d-bit, %d input sets; download of the picture at 43 GB/s: %.0f us" % (w, h, bd, a.sets, download_us))
        print("  %-46s %10s %12s %14s %8s" % ("entry", "us / call", "MB read", "us at 8 TB/s", "ratio"))
        rows = {}
        for name, nbytes, fn in entries:
            us = timed(fn, a.reps, a.sets)
            floor = nbytes / HBM_BPS * 1e6
            print("  %-46s %10.1f %12.1f %14.2f %8.1f" % (name, us, nbytes / 1e6, floor, us / floor))
            rows[name] = {"us": round(us, 2), "MB_read": round(nbytes / 1e6, 2), "us_at_8TBps": round(floor, 2), "ratio": round(us / floor, 2)}
        report["%dx%d" % (w, h)] = {"download_us": round(download_us, 1), "entries": rows}
        del sets
        torch.cuda.empty_cache()
    print(json.dumps(report))


if __name__ == "__main__":
    main()
