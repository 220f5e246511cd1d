#!/usr/bin/env python3
"""The intra mode pre-selection pass (IntraSearch::estIntraPredLumaQT, IntraSearch.cpp:405-522 and 591-618) of a 10-bit 3840x2160 picture:
  4K      every interior 16x16 block of the picture (the list of tools/intra_search_time.py);
  mix     about 8 000 PUs at random positions whose shapes follow the committed call trace (tests/golden/trace_ragop16_416x240_10b_q32.npz: the
          shapes of its pelop calls with sides 4..64).
Random MPMs (planar or DC among them in a third of the PUs), numModesForFullRD 3 (2 for 4x64 and 64x4), the PBINTRA gate on for every second PU.
  (a) the chained form (tests/intra_mode_cand_chain.py), built from entries the library already had: vvcgpu_intra_fill_refs_batch,
      vvcgpu_intra_satd_batch of 35 descriptors per PU (uploaded once, outside the timed part), download, the lists on the host (vectorised numpy),
      upload of the second round's descriptors, vvcgpu_intra_satd_batch, download, the lists' tail on the host;
  (b) vvcgpu_intra_mode_cand_batch and the download of its three outputs.
The results of (a) and (b) are compared before anything is timed.  Times: device events around a whole run on the stream (for (a) that includes the
host's part: it is what the caller waits for), 3 warm-up runs, then the median and the spread of 7 runs, (a) and (b) alternating.  The device time of
(a)'s three launches alone (without downloads and host lists) and of (b)'s one launch alone are given too, so that the kernels compare on their own."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import intra_mode_cand_cases as imc  # noqa: E402
import intra_mode_cand_chain as chain  # noqa: E402
import pu_search_kit as kit  # noqa: E402
import rd_pass_kit  # noqa: E402

W, H, BD = 3840, 2160, 10
SQRT_LAMBDA = 27.375
WARMUP, RUNS = 3, 7
rng = np.random.default_rng(41)


def build(rec, org, w, h, px, py):
    n = len(w)
    pus = np.zeros(n, imc.PU)
    pus["x"], pus["y"], pus["w"], pus["h"] = px, py, w, h
    mpm = np.stack([rng.permutation(imc.N_MODES)[:3] for _ in range(n)])
    low = rng.integers(0, 3, n) == 0
    mpm[low, rng.integers(0, 3, n)[low]] = rng.integers(0, 2, n)[low]
    clash = np.array([len(set(r)) < 3 for r in mpm])
    mpm[clash] = (0, 1, 50)
    pus["mpm"] = mpm
    pus["num_modes"] = np.where(((w == 4) & (h == 64)) | ((w == 64) & (h == 4)), 2, 3)
    one = 1 << 15
    f1, f0 = rng.integers(one // 4, 2 * one, n), rng.integers(one // 4, 2 * one, n)
    pus["bits"] = np.stack([f1 + one, f1 + 2 * one, f1 + 2 * one, f0 + 6 * one], 1)
    # interHad around the block's typical SATD: every branch of the cut is taken somewhere
    pus["inter_had"] = np.where(np.arange(n) % 2 == 0, np.uint64(imc.U64_MAX), (w * h * rng.integers(2, 40, n)).astype(np.uint64))
    lens = np.array([sum(imc.ref_lengths(int(a), int(b))) + 1 for a, b in zip(w, h)])
    pus["ref_off"] = np.concatenate([[0], np.cumsum(lens)[:-1]])
    pus["flags_off"] = 0                                                     # every unit available: one shared run of flags
    return imc.Case(rec, org, pus, np.ones(192, np.uint8), BD)


def main():
    rec = kit.texture(rng, H, W, BD, 0.0)
    org = np.clip(np.roll(rec, (1, -2), axis=(0, 1)).astype(np.int32) + rng.integers(-4, 5, (H, W)), 0, 1023).astype(np.int16)
    lists = rd_pass_kit.timing_lists(rng, W, H, imc.SIDES)                   # (the row has columns of its own: the launches alone, the final list sizes)
    print("list          PUs   chain ms (min..max)   its launches ms   entry ms (min..max)   its launch ms   chain / entry   launches / launch   final sizes 0 1 2 3+")
    for name, w, h, px, py in lists:
        D = chain.Device(build(rec, org, w, h, px, py))
        refs_a = D.fresh_refs()

        def entry():
            return chain.download(chain.run_entry(D, imc.USE_MPM, SQRT_LAMBDA, refs_a), None)

        def chained():
            return chain.run_chain(D, imc.USE_MPM, SQRT_LAMBDA)

        a, b = chained(), entry()
        assert np.array_equal(a["lists"], b["lists"]) and a["costs"].tobytes() == b["costs"].tobytes() and np.array_equal(a["satd"], b["satd"]), name
        assert np.array_equal(a["refs"], refs_a.cpu().numpy()), name
        ta, tb = kit.times_of_alternating((chained, entry), WARMUP - 1, RUNS)   # the comparison above was the first warm-up run
        tk = sorted(kit.events(lambda: chain.run_entry(D, imc.USE_MPM, SQRT_LAMBDA, refs_a))[0] for _ in range(RUNS))[RUNS // 2]
        dev = []
        for _ in range(RUNS):
            ms = []
            chain.run_chain(D, imc.USE_MPM, SQRT_LAMBDA, device_ms=ms)
            dev.append(sum(ms))
        td = sorted(dev)[RUNS // 2]
        ma, mb = float(np.median(ta)), float(np.median(tb))
        sizes = np.bincount(np.minimum(b["lists"][:, 0], 3), minlength=4)
        print("%-10s %6d   %8.2f (%.2f..%.2f)   %15.2f   %8.2f (%.2f..%.2f)   %13.2f   %13.2f   %17.2f   %s" %
              (name, len(w), ma, min(ta), max(ta), td, mb, min(tb), max(tb), tk, ma / mb, td / tk, " ".join(str(int(v)) for v in sizes)))


if __name__ == "__main__":
    main()
