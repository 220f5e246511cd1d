"""Times vvcgpu_alf_frame_stats and vvcgpu_alf_ctu_dist on the covariance records of a 4K picture (510 CTUs of 128x128) and of 1920x1080 (135 CTUs):
event-timed microseconds per call (calls queued back to back on one stream) on the 7x7 luma set, the 5x5 luma set and a chroma set, over record sets
that rotate (12 sets: a 4K picture's four sets are 24.5 MB, so no call finds its records in the 256 MiB last-level cache).  Beside each entry:
(a) a plain device read of the same bytes (torch.sum of the set), and (b) what the two entries replace -- the device-to-host copy of the four record
sets (into pinned memory, the best case) plus the int64 frame sums by numpy on the host, wall clock.  All CTUs are on (enable NULL): every record is
read.  Prints one table per picture size and one JSON line.  Usage: python tools/alf_decide_time.py [--reps 120] [--sets 12]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from vvcsoftware_vtm_amd import capi  # noqa: E402

SHAPES = [("luma 7x7", 25, 183, 1), ("luma 5x5", 25, 57, 0), ("chroma", 1, 57, 0)]


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
    rng = np.random.default_rng(3)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    call = capi.call
    report = {}
    for w, h in ((3840, 2160), (1920, 1080)):
        n = -(-w // 128) * -(-h // 128)
        rows, total_bytes = {}, 0
        print("%dx%d: %d CTUs of 128x128, %d record sets in rotation" % (w, h, n, a.sets))
        print("  %-34s %10s %10s %14s %8s" % ("entry", "us / call", "MB read", "plain read us", "ratio"))
        recs = {}
        for name, n_cls, n_vals, ft in SHAPES:
            N = 13 if ft else 7
            sets = [torch.randint(-(1 << 30), 1 << 30, (n, n_cls, n_vals), dtype=torch.int64, device="cuda") for _ in range(a.sets)]
            recs[name] = sets
            nbytes = n * n_cls * n_vals * 8
            total_bytes += nbytes * (2 if name == "chroma" else 1)
            coeff = np.ascontiguousarray(rng.integers(-60, 61, (25, N)), dtype=np.int32)
            idx = (np.arange(25) % 25).astype(np.int16)
            frame = torch.empty((n_cls, n_vals), dtype=torch.int64, device="cuda")
            dist = torch.empty((n, 2), dtype=torch.float64, device="cuda")
            ptrs = [capi.ptr(t) for t in sets]
            cp, ip = C.c_void_p(coeff.ctypes.data), C.c_void_p(idx.ctypes.data)
            plain = timed(lambda i: sets[i].sum(), a.reps, a.sets)
            entries = [
                ("alf_frame_stats", lambda i: call("vvcgpu_alf_frame_stats", ptrs[i], n, n_cls, n_vals, None, 0, capi.ptr(frame), st)),
                ("alf_ctu_dist", lambda i: call("vvcgpu_alf_ctu_dist", ptrs[i], n, n_cls, ft, cp, 25 if n_cls == 25 else 1, ip if n_cls == 25 else None, 10,
                                                 capi.ptr(dist), st)),
            ]
            for ename, fn in entries:
                us = timed(fn, a.reps, a.sets)
                key = "%s, %s" % (ename, name)
                print("  %-34s %10.1f %10.2f %14.1f %8.2f" % (key, us, nbytes / 1e6, plain, us / plain))
                rows[key] = {"us": round(us, 2), "MB_read": round(nbytes / 1e6, 2), "plain_read_us": round(plain, 2), "ratio_to_plain_read": round(us / plain, 2)}
        # (b) what the entries replace: all four record sets to the host, then the frame sums there
        four = [recs["luma 7x7"], recs["luma 5x5"], recs["chroma"], recs["chroma"]]
        host = [torch.empty(s[0].shape, dtype=torch.int64).pin_memory() for s in four]
        copy_us, sum_us = [], []
        for r in range(8):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for hbuf, s in zip(host, four):
                hbuf.copy_(s[r % a.sets], non_blocking=True)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            sums = [hbuf.numpy().sum(0, dtype=np.int64) for hbuf in host]
            t2 = time.perf_counter()
            assert len(sums) == 4
            if r >= 2:
                copy_us.append((t1 - t0) * 1e6)
                sum_us.append((t2 - t1) * 1e6)
        copy, hsum = float(np.median(copy_us)), float(np.median(sum_us))
        dev_all = sum(v["us"] for k, v in rows.items() if "chroma" not in k) + 2 * sum(v["us"] for k, v in rows.items() if "chroma" in k)
        print("  replaced: copy of the four sets to pinned host memory (%.1f MB) %.0f us (%.1f GB/s) + numpy int64 frame sums %.0f us = %.0f us" %
              (total_bytes / 1e6, copy, total_bytes / copy / 1e3, hsum, copy + hsum))
        print("  both entries on all four sets: %.1f us, %.0f x below what they replace" % (dev_all, (copy + hsum) / dev_all))
        for k, v in rows.items():
            v["replaced_over_entry"] = round((copy + hsum) / v["us"], 1)
        report["%dx%d" % (w, h)] = {"n_ctu": n, "entries": rows, "download_us": round(copy, 1), "host_sum_us": round(hsum, 1),
                                    "both_entries_all_sets_us": round(dev_all, 1), "replaced_over_both": round((copy + hsum) / dev_all, 1)}
        del recs, four
        torch.cuda.empty_cache()
    print(json.dumps(report))


if __name__ == "__main__":
    main()
