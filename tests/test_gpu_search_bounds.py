"""GPU parity where the integer searches' packed keys and the block distortions' sums are full: the planes and cost entries of
cases.search_bound_planes / SEARCH_BOUND_MVCOSTS / dist_bound_planes (tests/test_search_bounds_cpu.py asserts where they sit and checks the checker
there against numpy int64) through the hierarchical search, the six forms of vvcgpu_sad_search (dense9, dense, group, quad, pair, generic), the TZ search and vvcgpu_dist_batch, bit for bit
against the oracle.  With the fourth cost entry bit 31 of a raster key (cost << 2 | candidate) is set and lambda * bits uses 29 bits of the cost
table; with the tie planes every SAD is equal and the cost and the visiting order decide alone."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import cases
from oraclelib import oracle, p
from test_gpu_dist import SIZES
from test_gpu_mehier import grid_blocks, make, oracle_best
from test_gpu_tzsearch import run_gpu as tz_gpu, run_oracle as tz_oracle

pytestmark = pytest.mark.gpu

KINDS = tuple(cases.SEARCH_BOUND_KINDS)
bound_cases = pytest.mark.parametrize("kind,tie,ci", [(k, t, c) for k in KINDS for t in (False, True) for c in range(4)])


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()            # a copy: the cached planes are read-only


@functools.lru_cache(maxsize=None)
def planes(kind, tie, W, H, m):
    org, refp = cases.search_bound_planes(kind, tie, W, H, m)
    org.setflags(write=False), refp.setflags(write=False)
    return org, refp


def mvcost(row):
    from vvcsoftware_vtm_amd import ops
    return ops.MvCost(float(row[0]), int(row[1]), int(row[2]), 2, 0)


# ---- the hierarchical search ------------------------------------------------------------------------------------------------------------------------
def check_hier(org, refp, org_xy, ref_xy, n16x, n16y, ss, rr, dr, mv):
    from vvcsoftware_vtm_amd import ops
    raster, dense = ops.me_hier_search(dev(org), dev(refp), org_xy, ref_xy, n16x, n16y, ss, rr, dr, mv)
    nR = 2 * (rr // 5) + 1
    rgrid = (-5 * (rr // 5), -5 * (rr // 5), nR, nR, 5, 5)
    dgrid = (-dr, -dr, 2 * dr + 1, 2 * dr + 1, 1, 1)
    first, records = [], {}
    for k, s in enumerate((16, 32, 64)):
        blk = grid_blocks(n16x, n16y, s, org_xy, ref_xy)
        assert blk.size, s
        want = oracle_best(org, refp, blk, s, ss, rgrid, mv)
        got = raster[k].cpu().numpy().view(ops.SEARCH_BEST)
        assert np.array_equal(got, want), "raster %dx%d sub_shift %d" % (s, s, ss)
        records[s] = got
        first.append(np.all(got["x"] == rgrid[0]) and np.all(got["y"] == rgrid[1]))
        if dr:
            want = oracle_best(org, refp, blk, s, ss, dgrid, mv)
            got = dense[k].cpu().numpy().view(ops.SEARCH_BEST)
            assert np.array_equal(got, want), "dense %dx%d sub_shift %d" % (s, s, ss)
            first.append(np.all(got["x"] == -dr) and np.all(got["y"] == -dr))
    assert dr or dense is None
    return all(first), records                             # every winner is the first position; the raster records per block size


@bound_cases
def test_me_hier_at_the_key_bounds(kind, tie, ci):
    """one whole super-block and a partial column (5 x 4 blocks), raster 96 and +-4, both row steps"""
    m = 112
    org, refp = planes(kind, tie, 80, 64, m)
    for ss in (0, 1):
        first, _ = check_hier(org, refp, (0, 0), (m + 3, m - 2), 5, 4, ss, 96, 4, mvcost(cases.SEARCH_BOUND_MVCOSTS[ci]))
        assert first or not (tie and ci == 0)              # every cost equal: the first position in scan order wins everywhere


@pytest.mark.parametrize("n16x", [12, 36])
@pytest.mark.parametrize("tie", [False, True])
def test_me_hier_at_the_key_bounds_persistent_workgroups(monkeypatch, n16x, tie):
    """VVCGPU_MH_WGS = 8: 12 x 4 blocks are three super-blocks for eight workgroups (one each: mh_run_of gives runs of ceil(ceil(total / 8) / (wgs / 8)));
    36 x 4 are nine, so the workgroups of four XCDs walk two and SLIDE their window"""
    monkeypatch.setenv("VVCGPU_MH_WGS", "8")
    m = 112
    org, refp = planes("int16_lo", tie, 16 * n16x, 64, m)
    for ss in (0, 1):
        check_hier(org, refp, (0, 0), (m - 3, m + 1), n16x, 4, ss, 96, 4, mvcost(cases.SEARCH_BOUND_MVCOSTS[3]))


@pytest.mark.parametrize("rr,dr", [(99, 4), (20, 4), (5, 0)])
def test_me_hier_range_edges(rr, dr):
    """the ends of the accepted ranges: raster 99 (R = 95, 39 x 39), R = D + 16 (the dense grid's spans end at the window's edge), the 3 x 3 raster alone"""
    rng = np.random.default_rng(rr + dr)
    m = 112
    org, refp = make(rng, 80, 64, m, "smooth")
    for ss, ci in ((1, 2), (0, 1)):
        check_hier(org, refp, (0, 0), (m + 2, m + 1), 5, 4, ss, rr, dr, mvcost(cases.SEARCH_BOUND_MVCOSTS[ci]))


# ---- every form of vvcgpu_sad_search ------------------------------------------------------------------------------------------------------------------
SW, SH, SM = 256, 160, 120                                # picture and margin of the raster forms: 5 x 22 + 9 <= 120


def group_blocks(h):
    """the run layout of test_sad_search_group_runs, shortened: full and short runs, a run broken by a reference offset, a run on odd columns, isolated
    blocks, a ragged tail (30 blocks)"""
    from vvcsoftware_vtm_amd import ops
    rows = []

    def run(x0, y0, n, dx=0, dy=0):
        for t in range(n):
            rows.append((x0 + 16 * t, y0, SM + x0 + 16 * t + dx, SM + y0 + dy))
    run(0, 0, 8); run(128, 0, 5, 3, -2); run(208, 0, 3, -7, 5)
    run(0, 32, 3, 1, 1); rows.append((48, 32, SM + 48 + 2, SM + 32 + 1))
    run(64, 32, 2, 1, 2)
    run(33, 64, 6, 2, -3)
    rows.append((201, 40, SM + 201 - 9, SM + 40 + 9)); rows.append((118, 5, SM + 118 + 9, SM + 5 - 9))
    blk = np.array(rows, dtype=ops.SEARCH_BLK)
    assert blk.size == 30 and np.all(blk["org_y"] + h <= SH) and np.all(blk["org_x"] + 16 <= SW)
    return blk


def scattered_blocks(w, h, W, H, m, spread, n=5):
    """n blocks all over the picture, every third on an odd column (the original's sample-wise packing), reference offsets within +-spread"""
    from vvcsoftware_vtm_amd import ops
    rng = np.random.default_rng(w * 3 + h)
    blk = np.zeros(n, ops.SEARCH_BLK)
    for i in range(n):
        x, y = int(rng.integers(0, (W - w) // 2 + 1)) * 2, int(rng.integers(0, H - h + 1))
        if i % 3 == 2 and x + 1 + w <= W:
            x += 1
        blk[i] = (x, y, m + x + int(rng.integers(-spread, spread + 1)), m + y + int(rng.integers(-spread, spread + 1)))
    return blk


def check_sad(org, refp, blk, w, h, ss, grid, mv, surface):
    from vvcsoftware_vtm_amd import ops
    dx0, dy0, nx, ny, sx, sy = grid
    want = np.zeros((blk.size, ny, nx), np.uint32)
    wbest = np.zeros(blk.size, ops.SEARCH_BEST)
    oracle().orc_sad_search(p(org), org.shape[1], p(refp), refp.shape[1], p(blk), blk.size, w, h, ss, dx0, dy0, nx, ny, sx, sy, p(want), C.byref(mv), p(wbest))
    d_org, d_ref, d_blk = dev(org), dev(refp), ops.struct_to_device(blk)
    for want_sad in ((False, True) if surface == "both" else (surface,)):
        sad, best = ops.sad_search(d_org, d_ref, d_blk, blk.size, w, h, ss, dx0, dy0, nx, ny, sx, sy, mv, want_sad=want_sad)
        what = "%dx%d sub_shift %d grid %s surface %s" % (w, h, ss, grid, want_sad)
        assert (sad is not None) == want_sad
        if want_sad:
            assert np.array_equal(sad.cpu().numpy().view(np.uint32), want), what
        assert np.array_equal(best.cpu().numpy().view(ops.SEARCH_BEST), wbest), what
    return wbest


def raster_grid(nx, ny):
    return (-5 * (nx // 2), -5 * (ny // 2), nx, ny, 5, 5)


@bound_cases
def test_sad_search_group_form_at_the_key_bounds(kind, tie, ci):
    """16-wide blocks, best only, lambda < 4e6: sad_raster5gq_kernel, the 32-bit key"""
    org, refp = planes(kind, tie, SW, SH, SM)
    mv = mvcost(cases.SEARCH_BOUND_MVCOSTS[ci])
    for h in (16, 32):
        for (nx, ny, ss) in ((39, 39, 1), (20, 13, 0)):
            grid = raster_grid(nx, ny)
            best = check_sad(org, refp, group_blocks(h), 16, h, ss, grid, mv, False)
            if tie and ci == 0:
                assert np.all(best["x"] == grid[0]) and np.all(best["y"] == grid[1])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("tie", [False, True])
def test_sad_search_group_hands_over_beyond_its_key(kind, tie):
    """lambda >= 4e6: lambda * bits no longer fits the group form's key; the same call goes to the quad form's 64-bit key"""
    org, refp = planes(kind, tie, SW, SH, SM)
    for lam in (4.0e6, 2.0e7):
        for row in cases.SEARCH_BOUND_MVCOSTS[2:]:
            check_sad(org, refp, group_blocks(16), 16, 16, 1, raster_grid(39, 39), mvcost((lam,) + tuple(row[1:])), False)


@bound_cases
def test_sad_search_quad_form_at_the_key_bounds(kind, tie, ci):
    """sad_raster5q_kernel (grids of at most 40 columns), best only and with the surface; 128x128: SADs beyond 2^29 in the uint32 surface"""
    org, refp = planes(kind, tie, SW, SH, SM)
    mv = mvcost(cases.SEARCH_BOUND_MVCOSTS[ci])
    for (s, nx, ny) in ((32, 39, 39), (64, 39, 39), (128, 9, 7)):
        check_sad(org, refp, scattered_blocks(s, s, SW, SH, SM, 9), s, s, 0, raster_grid(nx, ny), mv, "both")


@bound_cases
def test_sad_search_pair_form_at_the_key_bounds(kind, tie, ci):
    """sad_raster5c_kernel: a raster wider than 40 columns"""
    org, refp = planes(kind, tie, SW, SH, SM)
    mv = mvcost(cases.SEARCH_BOUND_MVCOSTS[ci])
    for (s, ss) in ((16, 1), (64, 0)):
        check_sad(org, refp, scattered_blocks(s, s, SW, SH, SM, 9), s, s, ss, raster_grid(45, 23), mv, "both")


@bound_cases
def test_sad_search_dense9_form_at_the_key_bounds(kind, tie, ci):
    """sad_dense9_kernel: the +-4 grid of 16-multiple blocks under 2:1 row sub-sampling"""
    org, refp = planes(kind, tie, SW, SH, SM)
    mv = mvcost(cases.SEARCH_BOUND_MVCOSTS[ci])
    for s in (16, 32):
        check_sad(org, refp, scattered_blocks(s, s, SW, SH, SM, 9, n=7), s, s, 1, (-4, -4, 9, 9, 1, 1), mv, "both")


@bound_cases
def test_sad_search_dense_form_at_the_key_bounds(kind, tie, ci):
    """sad_dense_kernel: the step-1 grids that dense9 does not take -- 64x64 blocks, no row sub-sampling, 128- and 8-wide blocks, grids other than 9 x 9;
    its 64-bit key (SAD + lambda * bits) << 24 | position, the 32-bit SAD of a 128x128 block at 553 631 744"""
    org, refp = planes(kind, tie, SW, SH, SM)
    mv = mvcost(cases.SEARCH_BOUND_MVCOSTS[ci])
    for (s, ss, grid) in ((64, 1, (-4, -4, 9, 9, 1, 1)), (16, 0, (-4, -4, 9, 9, 1, 1)), (128, 0, (-4, -4, 9, 9, 1, 1)),
                          (32, 1, (-3, -2, 7, 5, 1, 1)), (8, 0, (-3, -2, 7, 5, 1, 1))):
        check_sad(org, refp, scattered_blocks(s, s, SW, SH, SM, 9, n=7), s, s, ss, grid, mv, "both")


@bound_cases
def test_sad_search_generic_form_at_the_key_bounds(kind, tie, ci):
    """sad_search_kernel: a reference stride that is no multiple of 8 (330, as test_sad_search_best_only_generic) and grids of step 3 / 5"""
    W, H, m = 250, 96, 40
    org, refp = planes(kind, tie, W, H, m)
    assert refp.shape[1] == 330
    mv = mvcost(cases.SEARCH_BOUND_MVCOSTS[ci])
    for (w, h, ss) in ((8, 8, 0), (12, 16, 1)):
        for grid in ((-6, -6, 5, 5, 3, 3), (-10, -10, 5, 5, 5, 5)):
            check_sad(org, refp, scattered_blocks(w, h, W, H, m, 5, n=7), w, h, ss, grid, mv, "both")


def test_raster_keys_on_both_sides_of_bit_31():
    """cases.search_bit31_planes: the winner's 32-bit key is below 2^31, the key of the next candidate of its lane above (the planes above put all keys of a
    block on one side) -- the 64x64 block of the hierarchical search for both row steps, a 16x128 block of the group form"""
    from vvcsoftware_vtm_amd import ops
    m = 112
    mv = mvcost(cases.SEARCH_BOUND_MVCOSTS[3])
    org, refp = cases.search_bit31_planes(15000, 64, 64, m, 0, 0, 64, 64)
    for ss in (0, 1):
        got = check_hier(org, refp, (0, 0), (m, m), 4, 4, ss, 96, 4, mv)[1][64][0]
        assert (got["x"], got["y"], got["cost"]) == (-5, 10, 61440000 - 4096 + 471999941)
    org, refp = cases.search_bit31_planes(30000, 16, 128, m, 0, 0, 16, 128)
    best = check_sad(org, refp, np.array([(0, 0, m, m)], ops.SEARCH_BLK), 16, 128, 0, raster_grid(39, 39), mv, False)
    assert (best["x"][0], best["y"][0], best["cost"][0]) == (-5, 10, 61440000 - 2048 + 471999941)


# ---- the TZ search ----------------------------------------------------------------------------------------------------------------------------------
TW, TH, TM = 256, 256, 160


def tz_bound_pus(sizes, row):
    """PUs in the interior and at two corners of the picture, the start vector at zero and away from it, plain and extended settings"""
    pus = []
    for (s, ss) in sizes:
        for (x, y) in ((64, 64), (0, 0), (TW - s, TH - s)):
            for (sx, sy) in ((0, 0), (60, -44)):
                for fl in (0, 2):
                    pus.append((x, y, TM + x, TM + y, sx, sy, 0, 0, x, y, row[1], row[2], s, s, ss, fl, (0, 0)))
    return np.array(pus, dtype=cases.TZ_PU)


@bound_cases
def test_tz_search_at_the_key_bounds(kind, tie, ci):
    """one-launch form (both team shapes, PUs of the three sizes in one batch) and split form (uniform 16x16 and 64x64 batches), search range 96"""
    org, refp = (a.copy() for a in planes(kind, tie, TW, TH, TM))
    row = cases.SEARCH_BOUND_MVCOSTS_TZ[ci]
    cfg = cases.tz_cfg(TW, TH, TM, row[0], search_range=96)
    pus = tz_bound_pus(((16, 1), (64, 1), (128, 0)), row)
    want = tz_oracle(org, refp, pus, cfg)
    got = tz_gpu(org, refp, pus, cfg)
    assert np.array_equal(got, want), np.nonzero(got != want)[0][:8]
    for s in (16, 64):
        pus = tz_bound_pus(((s, 1),), row)
        want = tz_oracle(org, refp, pus, cfg)
        cfg_split = cfg.copy()
        cfg_split["reserved"] = (s << 16) | s            # vvcgpu_tz_cfg.uniform_pu
        got = tz_gpu(org, refp, pus, cfg_split)
        assert np.array_equal(got, want), (s, np.nonzero(got != want)[0][:8])


# ---- the block distortions -----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def dist_bound_case(pat, bd):
    """every size of test_gpu_dist.SIZES as a block of dist_bound_planes in a 128-wide plane, one below the other -> org, cur, (y0, w, h) rows"""
    tot = sum(h for (_, h) in SIZES)
    org, cur = np.zeros((tot, 128), np.int16), np.zeros((tot, 128), np.int16)
    rows, y0 = [], 0
    for (w, h) in SIZES:
        org[y0:y0 + h, :w], cur[y0:y0 + h, :w] = cases.dist_bound_planes(pat, w, h, bd)
        rows.append((y0, w, h))
        y0 += h
    return org, cur, rows


@pytest.mark.parametrize("kind", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("pat", cases.DIST_BOUND_KINDS)
@pytest.mark.parametrize("bd", [8, 10])
def test_dist_batch_at_full_range(kind, pat, bd):
    from vvcsoftware_vtm_amd import ops
    org, cur, rows = dist_bound_case(pat, bd)
    d = []
    for (y0, w, h) in rows:
        for ss in ((0, 1) if kind in (ops.SAD, ops.MRSAD) and h >= 8 else (0,)):
            d.append((y0 * 128, y0 * 128, 128, 128, w, h, ss, 0))
    d = np.array(d, dtype=ops.DIST_DESC)
    want = np.zeros(len(d), np.uint64)
    oracle().orc_dist_batch(kind, p(org), p(cur), p(d), len(d), p(want))
    got = ops.dist_batch(kind, dev(org), dev(cur), ops.struct_to_device(d), len(d), bd).cpu().numpy().view(np.uint64)
    assert np.array_equal(got, want), np.nonzero(got != want)[0][:8]
    if kind == ops.SSE and pat == "const" and bd == 10:
        assert int(got.max()) == 17146331136
