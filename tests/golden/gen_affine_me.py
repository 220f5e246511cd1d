"""Generates tests/golden/affine_me.npz: whole affine motion searches by the COMPILED REFERENCE.  Build machine only (needs the reference tree and
oracle/_ref/libvtmref.so, i.e. a build() where the reference exists):  python tests/golden/gen_affine_me.py

Every search is the reference's own InterSearch::xAffineMotionEstimation, reached through gen_affine_me_driver.cpp, which is compiled here against the
reference's headers (the include set of oracle/Makefile's CXXFLAGS_REF, -fno-access-control) and linked with libvtmref.so.  Nothing of the reference
is copied; only the resulting data is stored.  Per bit depth (10, 8): one 256x128 reference plane (smooth texture plus noise, with a patch of vertical
stripes and a flat patch), an atlas of original blocks (the reference's own affine prediction with "true" vectors, plus noise, so that the searches
move; "2 org - other prediction" blocks for the half-weight searches), the items, each item's getUseAffineType, the motion lambda and the reference's
results.  The generator asserts that the set holds the cases the tests rely on; the per-search step counts it needs for that come from the tests'
restatement (tests/affine_me_cases.py) AFTER it has reproduced every one of the reference's results."""
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

import affine_me_cases as amc  # noqa: E402
import pu_search_kit as kit  # noqa: E402
from oraclelib import p  # noqa: E402
from vvcsoftware_vtm_amd import abi  # noqa: E402

REF = os.environ.get("REF", "/root/reference")
W, H = 256, 128
STRIPES = (128, 64, 64, 64)          # x, y, w, h of the vertical stripes; the flat patch is the 64 columns to its right
SIZES = [(16, 16), (32, 32), (64, 16), (16, 64), (64, 32), (128, 128), (16, 128), (128, 16), (48, 16), (16, 24)]


def driver():
    src = os.path.join(REF, "source", "Lib")
    inc = ["-I" + os.path.join(src, d) for d in ("", "CommonLib", "CommonLib/x86", "libmd5", "EncoderLib", "DecoderLib", "Utilities")]
    refdir = os.path.join(ROOT, "oracle", "_ref")
    out = os.path.join(tempfile.mkdtemp(), "libafmref.so")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-fPIC", "-shared", "-msse4.1", "-w", "-DNDEBUG", "-fno-access-control"] + inc +
                          [os.path.join(HERE, "gen_affine_me_driver.cpp"), "-o", out, "-L" + refdir, "-lvtmref", "-Wl,-rpath," + refdir])
    return C.CDLL(out)


def plane(rng, bd):
    a = kit.texture(rng, H, W, bd)
    x0, y0, w, h = STRIPES
    a[y0:y0 + h, x0:x0 + w] = ((np.arange(w) % 7) * ((1 << bd) // 9) + (1 << bd) // 8).astype(np.int16)[None, :]
    a[y0:y0 + h, x0 + w:] = (1 << bd) // 3
    return a


def ref_search(D, org, it):
    mv, mvp = np.ascontiguousarray(it["pu"]["mv"][0].reshape(-1)), np.ascontiguousarray(it["mvp"].reshape(-1))
    out_mv, out_bits, out_cost = np.zeros(6, np.int32), C.c_uint(0), C.c_uint64(0)
    blk = org.reshape(-1)[int(it["org_off"]):]
    D.afmref_search(p(blk), int(it["org_stride"]), int(it["pu"]["pos_x"]), int(it["pu"]["pos_y"]), int(it["pu"]["w"]), int(it["pu"]["h"]),
                    int(it["pu"]["six_param"]), int(it["half_weight"]), p(mv), p(mvp), int(it["bits"]), p(out_mv), C.byref(out_bits), C.byref(out_cost))
    r = np.zeros(1, abi.AFFINE_ME_RESULT)
    r[0]["mv"], r[0]["bits"], r[0]["cost"] = out_mv.reshape(3, 2), out_bits.value, out_cost.value
    return r[0]


def build_set(D, bd, rng):
    mx = (1 << bd) - 1
    lam = 37.5 if bd == 10 else 11.25
    ref = plane(rng, bd)
    atlas = np.zeros((0, W), np.int16)
    items, ats, tags = [], [], []

    def add_block(blk):
        nonlocal atlas
        h, w = blk.shape
        rows = np.zeros((h, W), np.int16)
        rows[:, :w] = blk
        off = atlas.shape[0] * W
        atlas = np.concatenate([atlas, rows])
        return off

    def warped(px, py, w, h, six, true_mv, noise):
        D.afmref_open(p(ref), W, H, bd, 1, C.c_double(lam))
        dst = np.zeros((h, w), np.int16)
        D.afmref_pred(px, py, w, h, int(six), p(np.ascontiguousarray(true_mv.reshape(-1))), p(dst))
        return np.clip(dst.astype(np.int32) + rng.integers(-noise, noise + 1, (h, w)), 0, mx).astype(np.int16)

    def add(tag, px, py, w, h, six, start, off, hw, at, mvp=None, bits=0):
        items.append(amc.item(px, py, w, h, six, start, off, W, hw, mvp if mvp is not None else start + rng.integers(-3, 4, (3, 2)) * 4, bits))
        ats.append(at)
        tags.append(tag)

    # the listed sizes: a warped original each; a uni search (4- or 6-parameter) and a half-weight search on "2 org - other" from the same block
    for k, (w, h) in enumerate(SIZES):
        px, py = (0, 0) if (w, h) == (128, 128) else (int(rng.integers(0, (W // 2 - w) // 4 + 1)) * 4, int(rng.integers(0, (H - h) // 4 + 1)) * 4)
        six = k % 2 == 1
        true_mv = amc.random_true_mv(rng, w, h, six, 24)
        o = warped(px, py, w, h, six, true_mv, 4)
        off = add_block(o)
        other = np.clip(o.astype(np.int32) + rng.integers(-9, 10, o.shape), 0, mx)
        off2 = add_block((2 * o.astype(np.int32) - other).astype(np.int16))
        start = true_mv + rng.integers(-6, 7, (3, 2)) * 4
        add("size", px, py, w, h, six, start, off, 0, 1, bits=int(rng.integers(0, 9)))
        add("size_hw", px, py, w, h, six, start, off2, 1, (k // 2) % 2)
        if k < 6:
            add("size_at0", px, py, w, h, not six, true_mv + rng.integers(-9, 10, (3, 2)) * 4, off, 0, 0)
    # a start far from the truth (long runs), and the truth itself with a predictor of its own (early stop)
    for k in range(3):
        w, h = [(32, 32), (64, 32), (16, 16)][k]
        px, py = int(rng.integers(0, 8)) * 4, int(rng.integers(0, 8)) * 4
        six = k == 1
        true_mv = amc.random_true_mv(rng, w, h, six, 16)
        off = add_block(warped(px, py, w, h, six, true_mv, 2))
        add("far", px, py, w, h, six, true_mv + rng.integers(-14, 15, (3, 2)) * 4, off, 0, 0)
        add("near", px, py, w, h, six, true_mv, off, 0, 1)
    # flat PU and vertical stripes (the noise-free reference patch itself is the original)
    sx, sy, sw, sh = STRIPES
    z = np.zeros((3, 2), np.int32)
    off = add_block(np.full((16, 16), mx // 3 + 5, np.int16))
    add("flat", sx + sw + 24, sy + 24, 16, 16, False, z, off, 0, 1)
    add("flat", sx + sw + 24, sy + 24, 16, 16, True, z, off, 0, 1)
    blk = ref[sy + 24:sy + 40, sx + 21:sx + 37].copy()
    off = add_block(blk)
    add("stripes", sx + 24, sy + 24, 16, 16, False, z + 4, off, 0, 1)
    add("stripes", sx + 24, sy + 24, 16, 16, True, z + 4, off, 0, 0)
    # corners, start vectors far outside: clipMv binds
    off = add_block(ref[0:32, 0:32].copy())
    add("corner", 0, 0, 32, 32, False, z - 4000, off, 0, 1, mvp=z)
    add("corner", 0, 0, 32, 32, True, np.array([[-4000, -3000], [-2000, -4000], [-5000, 200]], np.int32), off, 1, 1, mvp=z)
    off = add_block(ref[H - 16:H, W - 16:W].copy())
    add("corner", W - 16, H - 16, 16, 16, True, z + 4000, off, 0, 1, mvp=z)
    add("corner", W - 16, H - 16, 16, 16, False, np.array([[700, 4000], [800, 3000], [0, 0]], np.int32), off, 0, 0, mvp=z + 40)

    items = np.array(items, dtype=abi.AFFINE_ME_ITEM)
    ats = np.array(ats, np.int32)
    want = np.zeros(len(items), abi.AFFINE_ME_RESULT)
    for at in (1, 0):
        D.afmref_open(p(ref), W, H, bd, at, C.c_double(lam))
        for i in np.nonzero(ats == at)[0]:
            want[i] = ref_search(D, atlas, items[i])
    return ref, np.ascontiguousarray(atlas), items, ats, lam, want, tags


def check_set(bd, ref, atlas, items, ats, lam, want, tags):
    """the restatement reproduces every reference result; with its step counts: the set holds the cases the tests rely on"""
    refp = kit.pad(ref)
    steps, facts = np.zeros(len(items), np.uint32), set()
    for at in (1, 0):
        cfg = amc.make_cfg(lam, W, H, bd, at)
        idx = np.nonzero(ats == at)[0]
        res, trace = amc.search_all(atlas, refp, cfg, items[idx])
        for j, i in enumerate(idx):
            it, w = items[i], want[i]
            assert np.array_equal(res[j]["mv"], w["mv"]) and res[j]["bits"] == w["bits"] and res[j]["cost"] == w["cost"], (bd, i, tags[i], res[j], w)
            n = int(res[j]["steps"])
            steps[i] = n
            six, hw = bool(it["pu"]["six_param"]), bool(it["half_weight"])
            lim = 1 + amc.iter_limit(six, hw, at)
            facts.add(("six" if six else "four", "hw" if hw else "uni", at))
            facts.add(("size", int(it["pu"]["w"]), int(it["pu"]["h"])))
            if tags[i] == "flat":
                assert n == 1, (bd, i, n)
                facts.add("flat")
            elif tags[i] == "stripes":
                facts.add("stripes")
            elif tags[i] == "corner":
                nmv = 3 if six else 2
                assert not np.array_equal(trace[j][0]["mv"][:nmv], it["pu"]["mv"][0][:nmv]), (bd, i)       # clipMv moved the start vectors
                facts.add(("corner", int(it["pu"]["pos_x"]) == 0))
            else:
                if 1 < n < lim:
                    facts.add("early_zero_delta")
                if n == lim:
                    facts.add("to_the_limit")
                if n > 1 and trace[j][n - 1]["cost"] != res[j]["cost"]:
                    facts.add("best_is_not_last")
    for six in ("four", "six"):
        assert any(f[0] == six for f in facts if isinstance(f, tuple)), six
    for hw in ("uni", "hw"):
        for at in (1, 0):
            assert any(f[1:] == (hw, at) for f in facts if isinstance(f, tuple) and len(f) == 3 and f[0] in ("four", "six")), (hw, at)
    for f in ["flat", "stripes", "early_zero_delta", "to_the_limit", "best_is_not_last", ("corner", True), ("corner", False)] + \
            [("size", w, h) for w, h in SIZES]:
        assert f in facts, (bd, f, sorted(map(str, facts)))
    return steps


def main():
    D = driver()
    out = {}
    total = 0
    for bd in (10, 8):
        rng = np.random.default_rng(4100 + bd)
        ref, atlas, items, ats, lam, want, tags = build_set(D, bd, rng)
        steps = check_set(bd, ref, atlas, items, ats, lam, want, tags)
        want["steps"] = steps
        k = "bd%d_" % bd
        out.update({k + "ref": ref, k + "org": atlas, k + "items": items, k + "affine_type": ats, k + "lambda": np.float64(lam), k + "want": want})
        total += len(items)
        print("bit depth %d: %d searches, steps %s" % (bd, len(items), np.bincount(steps)))
    assert total >= 60
    path = os.path.join(HERE, "affine_me.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
