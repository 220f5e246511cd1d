"""Generates tests/golden/wp.npz: explicit weighted prediction by the COMPILED REFERENCE.  Build machine only (needs the reference tree and
oracle/_ref/libvtmref.so, i.e. a build() where the reference exists):  python tests/golden/gen_wp.py

The intermediates are the reference's own xPredInterBlk(..., bi = true) through vtmref_mc_batch with bi = 2; the weighting is the reference's own
WeightPrediction::addWeightUni / addWeightBi, reached through gen_wp_driver.cpp, which is compiled here against the reference's headers (the include
set of oracle/Makefile's CXXFLAGS_REF) and linked with libvtmref.so.  Nothing of the reference is copied; only the resulting data is stored.
Per bit depth: two reference planes ('extreme' content: outputs clip at both ends), the descriptors (reserved = table index), the table and the
expected output of every PU (dst_off / w / h of its descriptor, packed)."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

import cases  # noqa: E402
import wp_cases  # noqa: E402
from oraclelib import p, ref  # noqa: E402

REF = os.environ.get("REF", "/root/reference")


def driver():
    src = os.path.join(REF, "source", "Lib")
    inc = ["-I" + os.path.join(src, d) for d in ("", "CommonLib", "CommonLib/x86", "libmd5", "EncoderLib", "DecoderLib", "Utilities")]
    refdir = os.path.join(ROOT, "oracle", "_ref")
    out = os.path.join(tempfile.mkdtemp(), "libwpref.so")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-fPIC", "-shared", "-msse4.1", "-w", "-DNDEBUG"] + inc +
                          [os.path.join(HERE, "gen_wp_driver.cpp"), "-o", out, "-L" + refdir, "-lvtmref", "-Wl,-rpath," + refdir])
    return C.CDLL(out)


def main():
    R = ref()
    D = driver()
    out = {}
    for bd in (8, 10):
        rng = np.random.default_rng(700 + bd)
        mx = (1 << bd) - 1
        W, H = 96, 64
        r0, r1 = cases.rand_plane(rng, H, W, bd, "extreme"), cases.rand_plane(rng, H, W, bd, "extreme")
        uni, bi = wp_cases.wp_sets(bd)
        wp = wp_cases.table(uni + bi)
        ui, bix = list(range(len(uni))), list(range(len(uni), len(uni) + len(bi)))
        shapes = [(16, 16, 1), (8, 8, 1), (12, 4, 1), (8, 8, 0), (4, 4, 0), (2, 2, 0), (6, 4, 0)]
        d, n = wp_cases.pu_list(rng, W, H, shapes, 12, ui, bix)
        want = np.zeros(n, np.int16)
        for r, (p0, p1) in zip(d, wp_cases.intermediates(R.vtmref_mc_batch, r0, r1, d, bd)):
            e = wp[int(r["reserved"])]
            w, h = int(r["w"]), int(r["h"])
            o = np.zeros((h, w), np.int16)
            q1 = p1 if p1 is not None else p0
            D.wpref_apply(p(np.ascontiguousarray(p0)), p(np.ascontiguousarray(q1)), p(o), w, h, int(r["bi"]), int(e["w0"]), int(e["w1"]),
                          int(e["offset"]), int(e["shift"]), bd, 0, mx)
            want[int(r["dst_off"]):int(r["dst_off"]) + w * h] = o.reshape(-1)
        k = "bd%d_" % bd
        out.update({k + "r0": r0, k + "r1": r1, k + "descs": d, k + "wp": wp, k + "want": want})
    np.savez_compressed(os.path.join(HERE, "wp.npz"), **out)
    print("wrote", os.path.join(HERE, "wp.npz"), os.path.getsize(os.path.join(HERE, "wp.npz")), "bytes")


if __name__ == "__main__":
    main()
