"""GPU parity: the hierarchical integer search (vvcgpu_me_hier_search: step-5 raster + +-4 grid of every 16x16 / 32x32 / 64x64 block of a grid in one
launch, each 16x16 SAD computed once) against the oracle's per-block search (orc_sad_search, pinned by tests/golden/dist.npz against the compiled
reference), block size by block size -- bit-exact records (x, y, cost, sad), ties in visiting order."""
import ctypes as C

import numpy as np
import pytest
import torch

import cases
from oraclelib import oracle, p

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def grid_blocks(n16x, n16y, s, org_xy, ref_xy):
    from vvcsoftware_vtm_amd import ops
    k = s // 16
    nx, ny = n16x // k, n16y // k
    gx, gy = np.meshgrid(np.arange(nx) * s, np.arange(ny) * s)
    blk = np.zeros(nx * ny, ops.SEARCH_BLK)
    blk["org_x"], blk["org_y"] = gx.reshape(-1) + org_xy[0], gy.reshape(-1) + org_xy[1]
    blk["ref_x"], blk["ref_y"] = gx.reshape(-1) + ref_xy[0], gy.reshape(-1) + ref_xy[1]
    return blk


def oracle_best(org, refp, blk, s, ss, grid, mv):
    from vvcsoftware_vtm_amd import ops
    dx0, dy0, nx, ny, sx, sy = grid
    want = np.zeros((blk.size, ny, nx), np.uint32)
    wbest = np.zeros(blk.size, ops.SEARCH_BEST)
    oracle().orc_sad_search(p(org), org.shape[1], p(refp), refp.shape[1], p(blk), blk.size, s, s, ss, dx0, dy0, nx, ny, sx, sy, p(want), C.byref(mv), p(wbest))
    return wbest


def make(rng, W, H, m, content, bd=10):
    PW, PH = W + 2 * m, H + 2 * m
    if content == "flat":
        return np.full((H, W), 400, np.int16), np.full((PH, PW), 391, np.int16)
    if content == "ties":           # two-level planes: many positions share a SAD; the motion cost and the visiting order decide
        return (rng.integers(0, 2, (H, W)) * 64 + 300).astype(np.int16), (rng.integers(0, 2, (PH, PW)) * 64 + 300).astype(np.int16)
    if content == "bipred":         # 2 * org - otherPred: values outside the sample range, negatives included
        o = (2 * cases.rand_plane(rng, H, W, bd, "smooth").astype(np.int32) - cases.rand_plane(rng, H, W, bd, "smooth")).astype(np.int16)
        return o, cases.rand_plane(rng, PH, PW, bd, "smooth")
    if content == "moved":          # the original is the reference displaced by a per-region vector + noise: real minima inside the window
        refp = cases.rand_plane(rng, PH, PW, bd, "uniform")
        o = np.zeros((H, W), np.int16)
        for y0 in range(0, H, 64):
            for x0 in range(0, W, 64):
                dx, dy = int(rng.integers(-90, 91)), int(rng.integers(-90, 91))
                hh, ww = min(64, H - y0), min(64, W - x0)
                o[y0:y0 + hh, x0:x0 + ww] = refp[m + y0 + dy:m + y0 + dy + hh, m + x0 + dx:m + x0 + dx + ww]
        return np.clip(o + rng.integers(-3, 4, o.shape), 0, 1023).astype(np.int16), refp
    return cases.rand_plane(rng, H, W, bd, content), cases.rand_plane(rng, PH, PW, bd, content)


@pytest.mark.parametrize("n16x,n16y,ss,rr,dr,content,org_xy", [
    (13, 7, 1, 96, 4, "smooth", (0, 0)),          # partial super-blocks in both directions (13 = 3 x 4 + 1, 7 = 4 + 3)
    (8, 8, 1, 96, 4, "moved", (0, 0)),
    (8, 4, 1, 96, 4, "ties", (0, 0)),
    (4, 8, 1, 96, 4, "flat", (0, 0)),
    (9, 6, 0, 96, 4, "bipred", (0, 0)),           # no row sub-sampling
    (6, 5, 1, 64, 3, "smooth", (16, 32)),         # smaller raster (25 x 25), +-3 grid, grid origin inside the picture
    (5, 4, 1, 96, 0, "uniform", (2, 0)),          # raster only; original rows 4-byte but not 8-byte aligned
    (4, 4, 1, 30, 2, "moved", (0, 0)),
    (1, 1, 1, 96, 4, "smooth", (0, 0)),           # a grid without 32 / 64 blocks
    (3, 2, 1, 96, 4, "smooth", (0, 0)),
])
def test_me_hier_matches_per_block_search(n16x, n16y, ss, rr, dr, content, org_xy):
    from vvcsoftware_vtm_amd import ops
    rng = np.random.default_rng(n16x * 31 + n16y * 7 + ss + rr + dr)
    m = 112
    W, H = 16 * n16x + org_xy[0] + 8, 16 * n16y + org_xy[1] + 8
    W += (-W) % 8
    org, refp = make(rng, W, H, m, content)
    ref_xy = (m + org_xy[0] + int(rng.integers(-3, 4)), m + org_xy[1] + int(rng.integers(-3, 4)))
    lam = 0.0 if content == "flat" and n16x == 4 else float(rng.uniform(0.5, 90))
    mv = ops.MvCost(lam, int(rng.integers(-60, 60)), int(rng.integers(-60, 60)), 2, 0)
    raster, dense = ops.me_hier_search(dev(org), dev(refp), org_xy, ref_xy, n16x, n16y, ss, rr, dr, mv)
    nR = 2 * (rr // 5) + 1
    rgrid = (-5 * (rr // 5), -5 * (rr // 5), nR, nR, 5, 5)
    dgrid = (-dr, -dr, 2 * dr + 1, 2 * dr + 1, 1, 1)
    for k, s in enumerate((16, 32, 64)):
        blk = grid_blocks(n16x, n16y, s, org_xy, ref_xy)
        if blk.size == 0:
            assert raster[k] is None
            continue
        want = oracle_best(org, refp, blk, s, ss, rgrid, mv)
        got = raster[k].cpu().numpy().view(ops.SEARCH_BEST)
        assert np.array_equal(got, want), "raster %dx%d" % (s, s)
        if dr:
            want = oracle_best(org, refp, blk, s, ss, dgrid, mv)
            got = dense[k].cpu().numpy().view(ops.SEARCH_BEST)
            assert np.array_equal(got, want), "dense %dx%d" % (s, s)
    assert dr or dense is None


def test_me_hier_equals_the_per_size_kernels_1080p():
    """a whole 1920x1080 picture (grid 120 x 67: the last super-block row holds three rows of 16x16 blocks, one of 32x32 and no 64x64 block) against the
    per-size search kernels, which the oracle pins block by block (tests/test_gpu_dist.py)"""
    from vvcsoftware_vtm_amd import ops
    rng = np.random.default_rng(77)
    W, H, m = 1920, 1080, 144
    org, refp = make(rng, W, H, m, "moved")
    mv = ops.MvCost(7.55, 3, -2, 2, 0)
    d_org, d_ref = dev(org), dev(refp)
    n16x, n16y = W // 16, H // 16
    raster, dense = ops.me_hier_search(d_org, d_ref, (0, 0), (m, m), n16x, n16y, 1, 96, 4, mv)
    for k, s in enumerate((16, 32, 64)):
        blk = grid_blocks(n16x, n16y, s, (0, 0), (m, m))
        d_blk = ops.struct_to_device(blk)
        _, want = ops.sad_search(d_org, d_ref, d_blk, blk.size, s, s, 1, -95, -95, 39, 39, 5, 5, mv, want_sad=False)
        assert torch.equal(raster[k], want), "raster %d" % s
        _, want = ops.sad_search(d_org, d_ref, d_blk, blk.size, s, s, 1, -4, -4, 9, 9, 1, 1, mv, want_sad=False)
        assert torch.equal(dense[k], want), "dense %d" % s
    # the displaced content has its minima away from the centre: the raster must have found them
    got = raster[2].cpu().numpy().view(ops.SEARCH_BEST)
    assert (np.abs(got["x"]) > 4).mean() > 0.5


@pytest.mark.parametrize("n16x,n16y,rr,dr,org_xy,ref_dx", [
    (81, 8, 96, 4, (0, 0), 0),        # 21 super-blocks per row, the last one a single column of blocks: runs of 6 slide five times, the partial one refills
    (64, 12, 96, 4, (16, 0), 3),      # window origin 3 samples off a 16-byte boundary, grid origin inside the picture
    (48, 9, 64, 3, (0, 16), -2),      # smaller raster (25 x 25: fewer quads per window row), +-3 grid, partial last super-block row
])
def test_me_hier_sliding_window_runs(monkeypatch, n16x, n16y, rr, dr, org_xy, ref_dx):
    """eight persistent workgroups (VVCGPU_MH_WGS) over a wide grid: every workgroup walks a run of horizontally consecutive super-blocks and SLIDES its LDS
    window (mehier.hip); results against the per-size search kernels, which the oracle pins block by block (tests/test_gpu_dist.py)"""
    from vvcsoftware_vtm_amd import ops
    monkeypatch.setenv("VVCGPU_MH_WGS", "8")
    rng = np.random.default_rng(n16x + 3 * n16y + rr)
    m = 144
    W, H = 16 * n16x + org_xy[0], 16 * n16y + org_xy[1]
    W += (-W) % 8
    org, refp = make(rng, W, H, m, "moved")
    ref_xy = (m + org_xy[0] + ref_dx, m + org_xy[1] + 1)
    mv = ops.MvCost(11.25, -5, 9, 2, 0)
    d_org, d_ref = dev(org), dev(refp)
    raster, dense = ops.me_hier_search(d_org, d_ref, org_xy, ref_xy, n16x, n16y, 1, rr, dr, mv)
    R, nR = 5 * (rr // 5), 2 * (rr // 5) + 1
    for k, s in enumerate((16, 32, 64)):
        blk = grid_blocks(n16x, n16y, s, org_xy, ref_xy)
        d_blk = ops.struct_to_device(blk)
        _, want = ops.sad_search(d_org, d_ref, d_blk, blk.size, s, s, 1, -R, -R, nR, nR, 5, 5, mv, want_sad=False)
        assert torch.equal(raster[k], want), "raster %d" % s
        _, want = ops.sad_search(d_org, d_ref, d_blk, blk.size, s, s, 1, -dr, -dr, 2 * dr + 1, 2 * dr + 1, 1, 1, mv, want_sad=False)
        assert torch.equal(dense[k], want), "dense %d" % s


def test_me_hier_unsupported_shapes_are_refused():
    from vvcsoftware_vtm_amd import capi, ops
    org, refp = dev(np.zeros((64, 64), np.int16)), dev(np.zeros((400, 400), np.int16))
    for kw in (dict(raster_range=128), dict(dense_range=5), dict(sub_shift=2),
               dict(raster_range=100),                        # 41 x 41 positions
               dict(raster_range=15),                         # R < D + 15: the +-4 grid's spans would leave the window
               dict(lam=4.0e6)):                              # lambda * bits no longer below 2^29: the 32-bit raster key
        a = dict(sub_shift=1, raster_range=96, dense_range=4, lam=4.0)
        a.update(kw)
        with pytest.raises(capi.VvcGpuError, match="-3"):
            ops.me_hier_search(org, refp, (0, 0), (150, 150), 4, 4, a["sub_shift"], a["raster_range"], a["dense_range"], ops.MvCost(a["lam"], 0, 0, 2, 0))
    # the last lambda below the limit is served
    raster, dense = ops.me_hier_search(org, refp, (0, 0), (150, 150), 4, 4, 1, 96, 4, ops.MvCost(3999999.5, 0, 0, 2, 0))
    torch.cuda.synchronize()
    assert raster[2] is not None and dense[2] is not None
