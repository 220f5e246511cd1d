"""GPU parity of explicit weighted prediction (vvcgpu_mc_wp_batch), bit-exact: the reference's addWeightUni / addWeightBi (tests/golden/wp.npz), and
the restatement of tests/wp_cases.py on the reference's bi = 2 intermediates for every phase, shape, path and a picture's PU list."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import cases
import wp_cases
from oraclelib import oracle, ref, ref_available

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def mc_checker():
    """the bi = 2 intermediates: the compiled reference where it was built, else the CPU restatement that tests/test_oracle_golden.py pins to it"""
    return ref().vtmref_mc_batch if ref_available() else oracle().orc_mc_batch


def run_wp(r0, r1, d, wp, bd, lo, hi, dst0):
    from vvcsoftware_vtm_amd import ops
    got = dev(dst0)
    ops.mc_wp_batch(dev(r0), dev(r1), got, ops.struct_to_device(d), len(d), ops.struct_to_device(wp), len(wp), bd, (lo, hi))
    return got.cpu().numpy()


def check(r0, r1, d, wp, bd, lo, hi, n, poison=-5, want=None):
    dst0 = np.full(n, poison, np.int16)
    if want is None:
        want = wp_cases.expected(mc_checker(), r0, r1, d, wp, bd, lo, hi, dst0)
    got = run_wp(r0, r1, d, wp, bd, lo, hi, dst0)
    if not np.array_equal(got, want):
        bad = [i for i, r in enumerate(d) if not np.array_equal(got[r["dst_off"]:r["dst_off"] + r["w"] * r["h"]], want[r["dst_off"]:r["dst_off"] + r["w"] * r["h"]])]
        raise AssertionError("%d of %d PUs differ, first: %s" % (len(bad), len(d), [tuple(d[i]) for i in bad[:4]]))


@pytest.mark.ref
@pytest.mark.parametrize("bd", [8, 10])
def test_wp_golden(bd):
    g = np.load(os.path.join(G, "wp.npz"))
    k = "bd%d_" % bd
    d, want = g[k + "descs"], g[k + "want"]
    check(g[k + "r0"], g[k + "r1"], d, g[k + "wp"], bd, 0, (1 << bd) - 1, want.size, want=want)


@pytest.mark.ref
@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("kind", ["extreme", "smooth"])
def test_wp_every_phase(bd, kind):
    """every luma phase pair (16x16) and chroma phase pair (8x8), uni and bi, shuffled: the matrix-core path on the quarter / eighth grid, the generic
    body on the other phases -- with the WP sets of wp_cases.wp_sets; odd count (a trailing single chroma PU)"""
    rng = np.random.default_rng(31 * bd + len(kind))
    W, H, M = 384, 200, 8
    r0, r1 = cases.rand_plane(rng, H, W, bd, kind), cases.rand_plane(rng, H, W, bd, kind)
    uni, bi = wp_cases.wp_sets(bd)
    wp = wp_cases.table(uni + bi)
    rows = []
    for (w, luma, nf) in [(16, 1, 16), (8, 0, 32)]:
        for fx in range(nf):
            for fy in range(nf):
                for b in (0, 1):
                    x0, y0 = int(rng.integers(M, W - w - M)), int(rng.integers(M, H - w - M))
                    x1, y1 = int(rng.integers(M, W - w - M)), int(rng.integers(M, H - w - M))
                    q = 4
                    fx1, fy1 = (fx + q * int(rng.integers(0, nf // q))) % nf, (fy + q * int(rng.integers(0, nf // q))) % nf
                    ix = len(uni) + int(rng.integers(0, len(bi))) if b else int(rng.integers(0, len(uni)))
                    rows.append([y0 * W + x0, y1 * W + x1, 0, W, W, w, w, w, fx, fy, fx1, fy1, luma, b, ix])
    rows.append(rows[700][:])
    doff = 3
    out = []
    for k in rng.permutation(len(rows)):
        r = rows[k]
        r[2] = doff
        doff += r[6] * r[7]
        out.append(tuple(r))
    d = np.array(out, dtype=wp_cases.MC_DESC)
    check(r0, r1, d, wp, bd, 0, (1 << bd) - 1, doff)


@pytest.mark.ref
@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("W,doff0", [(384, 0), (387, 3)])      # odd reference stride / unaligned dst rows: the generic body
def test_wp_shapes_and_paths(bd, W, doff0):
    rng = np.random.default_rng(bd * 1000 + W)
    H = 320
    r0, r1 = cases.rand_plane(rng, H, W, bd, "smooth"), cases.rand_plane(rng, H, W, bd, "uniform")
    uni, bi = wp_cases.wp_sets(bd)
    wp = wp_cases.table(uni + bi)
    sides = [4, 8, 12, 16, 24, 32, 48, 64, 128]
    shapes = [(s, t, 1) for s in sides for t in (s, 8)] + [(s, t, 0) for s in [2] + sides[:-1] for t in (s, 4)]
    d, n = wp_cases.pu_list(rng, W, H, shapes, 2, list(range(len(uni))), list(range(len(uni), len(uni) + len(bi))), doff=doff0)
    check(r0, r1, d, wp, bd, 0, (1 << bd) - 1, n)


@pytest.mark.ref
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 7, 9])
def test_wp_few_pus(n):
    rng = np.random.default_rng(n)
    bd, W, H = 10, 256, 96
    r0, r1 = cases.rand_plane(rng, H, W, bd, "smooth"), cases.rand_plane(rng, H, W, bd, "uniform")
    uni, bi = wp_cases.wp_sets(bd)
    wp = wp_cases.table(uni + bi)
    for shapes in ([(16, 16, 1)], [(8, 8, 0)], [(16, 16, 1), (8, 8, 0)]):
        d, doff = wp_cases.pu_list(rng, W, H, shapes * n, 1, list(range(len(uni))), list(range(len(uni), len(uni) + len(bi))), quarter=True)
        d = d[:n]
        check(r0, r1, d, wp, bd, 0, 1023, doff)


@pytest.mark.ref
def test_wp_long_mixed_list():
    """>= 20k PUs, matrix-core and generic PUs interleaved at random"""
    rng = np.random.default_rng(43)
    bd, W, H, M = 10, 512, 384, 8
    r0, r1 = cases.rand_plane(rng, H, W, bd, "smooth"), cases.rand_plane(rng, H, W, bd, "uniform")
    uni, bi = wp_cases.wp_sets(bd)
    wp = wp_cases.table(uni + bi)
    shapes = [(16, 16, 1), (8, 8, 0), (4, 4, 1), (8, 8, 1), (4, 8, 1), (16, 8, 1), (4, 4, 0), (32, 32, 1), (2, 2, 0), (16, 16, 0)]
    pick = rng.choice(len(shapes), 21000, p=[0.35, 0.25, 0.1, 0.06, 0.05, 0.05, 0.05, 0.03, 0.03, 0.03])
    rows, doff = [], 0
    for k in pick:
        w, h, luma = shapes[k]
        nf = 16 if luma else 32
        q = 4 if rng.random() < 0.7 else 1
        b = int(rng.integers(0, 2))
        ix = len(uni) + int(rng.integers(0, len(bi))) if b else int(rng.integers(0, len(uni)))
        x0, y0 = int(rng.integers(M, W - w - M)), int(rng.integers(M, H - h - M))
        x1, y1 = int(rng.integers(M, W - w - M)), int(rng.integers(M, H - h - M))
        fr = [q * int(v) for v in rng.integers(0, nf // q, 4)]
        rows.append((y0 * W + x0, y1 * W + x1, doff, W, W, w, w, h, fr[0], fr[1], fr[2], fr[3], luma, b, ix))
        doff += w * h
    check(r0, r1, np.array(rows, dtype=wp_cases.MC_DESC), wp, bd, 0, 1023, doff)


@pytest.mark.parametrize("bd", [8, 10])
def test_wp_default_weights_equal_the_unweighted_prediction(bd):
    """bi with w = 1 << d, offset 0 == mc_picture_batch bi = 1; uni with default weights == bi = 0 (fractional phases, and full-sample positions of
    in-range samples)"""
    from vvcsoftware_vtm_amd import ops
    rng = np.random.default_rng(5 + bd)
    W, H = 384, 200
    mx = (1 << bd) - 1
    r0, r1 = cases.rand_plane(rng, H, W, bd, "extreme"), cases.rand_plane(rng, H, W, bd, "smooth")
    for den in (0, 3, 7):
        wp = wp_cases.table([ops.wp_param(bd, den, 1 << den, 0), ops.wp_param(bd, den, 1 << den, 0, 1 << den, 0)])
        shapes = [(16, 16, 1), (8, 8, 0), (24, 8, 1), (4, 4, 0), (32, 32, 1)]
        d, n = wp_cases.pu_list(rng, W, H, shapes, 40, [0], [1], quarter=den == 3)
        plain = d.copy()
        plain["reserved"] = 0
        want = torch.full((n,), -5, dtype=torch.int16, device="cuda")
        ops.mc_picture_batch(dev(r0), dev(r1), want, ops.struct_to_device(plain), len(plain), bd, (0, mx))
        got = run_wp(r0, r1, d, wp, bd, 0, mx, np.full(n, -5, np.int16))
        assert np.array_equal(got, want.cpu().numpy()), den


@pytest.mark.parametrize("bd", [8, 10])
def test_wp_skipped_descriptors_leave_dst_untouched(bd):
    """a bad table index, bi = 2, w / h outside 1..128 or an entry outside the WPScalingParam range: dst keeps its poison; the valid neighbours in the
    same list (both kernels' walks: 16x16 luma, 8x8 chroma pairs, generic shapes) are still right"""
    rng = np.random.default_rng(77 + bd)
    W, H = 384, 256
    r0, r1 = cases.rand_plane(rng, H, W, bd, "smooth"), cases.rand_plane(rng, H, W, bd, "smooth")
    top = 2 << bd
    good = [(64, 0, 3, 6), (64, 64, -5, 7)]
    bad = [(256, 0, 0, 6), (-256, 0, 0, 6), (1, 0, 0, 9), (1, 0, 0, -1), (64, 0, top + 1, 6), (64, 0, -top - 1, 6),
           (64, 256, 0, 7), (64, -256, 0, 7)]
    wp = wp_cases.table(good + bad)
    d, n = wp_cases.pu_list(rng, W, H, [(16, 16, 1), (8, 8, 0), (12, 8, 1), (8, 8, 0)], 24, [0], [1], quarter=True)
    k = np.arange(len(d))
    sel = k % 3 == 1
    d["reserved"][sel & (d["bi"] == 0)] = 2 + (k[sel & (d["bi"] == 0)] % 6)                     # uni entries outside the range
    d["reserved"][sel & (d["bi"] == 1)] = 8 + (k[sel & (d["bi"] == 1)] % 2)                      # w1 outside the range
    d["reserved"][k % 11 == 5] = len(wp)                                                          # index outside the table
    d["reserved"][k % 13 == 6] = -1
    d["bi"][k % 17 == 8] = 2
    d["bi"][k % 19 == 9] = -1
    d["h"][k == 3] = 0
    check(r0, r1, d, wp, bd, 0, (1 << bd) - 1, n, poison=-7)


@pytest.mark.ref
def test_wp_picture_pu_list():
    """the PU list of Workload(416, 240) (mc_pic: 16x16 luma, 8x8 chroma) with a seeded per-PU table index: 2 lists x 4 references x 3 components"""
    from vvcsoftware_vtm_amd.workload import Workload
    wl = Workload(416, 240)
    bd, mx = wl.bd, wl.mx
    rng = np.random.default_rng(2026)

    def flat(offs, arrs):
        buf = np.zeros(offs[-1], np.int16)
        for o, a in zip(offs, arrs):
            buf[o:o + a.size] = np.ascontiguousarray(a).reshape(-1)
        return buf
    r0, r1 = flat(wl.ref_plane_off, wl.ref0_pad), flat(wl.ref_plane_off, wl.ref1_pad)
    from vvcsoftware_vtm_amd import ops
    uni = [ops.wp_param(bd, 6, int(rng.integers(-128, 128)), int(rng.integers(-128, 128))) for _ in range(2 * 4 * 3)]      # [list][ref][comp]
    bi = [ops.wp_param(bd, 6, int(rng.integers(-128, 128)), int(rng.integers(-128, 128)), int(rng.integers(-128, 128)), int(rng.integers(-128, 128)))
          for _ in range(4 * 4 * 3)]                                                                                       # [ref0][ref1][comp]
    wp = wp_cases.table(uni + bi)
    d = wl.mc_pic.copy()
    comp = np.where(d["is_luma"] == 1, 0, 1 + rng.integers(0, 2, len(d)))
    ref0, ref1, lst = rng.integers(0, 4, len(d)), rng.integers(0, 4, len(d)), rng.integers(0, 2, len(d))
    d["reserved"] = np.where(d["bi"] == 1, 24 + (ref0 * 4 + ref1) * 3 + comp, (lst * 4 + ref0) * 3 + comp)
    check(r0, r1, d, wp, bd, 0, mx, wl.pic_plane_off[-1])


def test_wp_generic_body_takes_every_pu():
    """VVCGPU_NO_MFMA=1: the generic body (its packed tiles and the sample-wise form) serves every PU, matrix-core shapes included"""
    env = dict(os.environ, VVCGPU_NO_MFMA="1")
    sel = ["tests/test_gpu_mc_wp.py::test_wp_every_phase", "tests/test_gpu_mc_wp.py::test_wp_few_pus",
           "tests/test_gpu_mc_wp.py::test_wp_skipped_descriptors_leave_dst_untouched"]
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", "-p", "no:cacheprovider"] + sel, cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert " passed" in r.stdout
