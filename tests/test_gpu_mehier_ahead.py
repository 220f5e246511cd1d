"""GPU parity of the hierarchical search with the packed original rows touched a super-block ahead (mehier.hip, mh_touch.h): small grids whose runs of
super-blocks are a single item, one to three items long, wrap to the next row of super-blocks, end in a partial last column or row, or are shorter for the
last workgroups -- with eight persistent workgroups (VVCGPU_MH_WGS=8) and with the default count -- against the oracle's per-block search
(orc_sad_search), record for record as in tests/test_gpu_mehier.py.

With eight workgroups a run is ceil(super-blocks / 8) items: the grids up to 8 x 9 blocks give runs of one item (4x4: a single item in all; 5x4, 9x5,
13x3: a partial last column; 9x5, 13x3, 8x9: a partial last row); 20x9 gives runs of two that wrap (5 super-blocks per row) and a shorter last run (15
super-blocks); 17x13 runs of three that wrap, both partial edges, a shorter last run and a workgroup without any item (20 super-blocks)."""
import functools

import numpy as np
import pytest
import torch

from test_gpu_mehier import dev, grid_blocks, make, oracle_best

pytestmark = pytest.mark.gpu

M = 112
GRIDS = [(4, 4, 0), (5, 4, 2), (9, 5, -2), (13, 3, 3), (8, 9, 1), (20, 9, 5), (17, 13, 4)]   # (n16x, n16y, ref_dx): every ref_dx gives a window origin off a 16-byte boundary


@functools.lru_cache(maxsize=None)
def case(n16x, n16y, ref_dx, ss):
    """inputs and the oracle's records of one grid: computed once, shared by the workgroup counts"""
    from vvcsoftware_vtm_amd import ops
    rng = np.random.default_rng(1000 * n16x + 10 * n16y + ss)
    W, H = 16 * n16x + 8, 16 * n16y + 8
    W += (-W) % 8
    org, refp = make(rng, W, H, M, "moved")
    ref_xy = (M + ref_dx, M + 1)
    assert ((ref_xy[1] - 95) * refp.shape[1] + ref_xy[0] - 95) % 8 != 0            # a non-zero `off`
    mv = ops.MvCost(float(rng.uniform(0.5, 90)), int(rng.integers(-60, 60)), int(rng.integers(-60, 60)), 2, 0)
    want = {}
    for s in (16, 32, 64):
        blk = grid_blocks(n16x, n16y, s, (0, 0), ref_xy)
        if blk.size:
            want[s] = (oracle_best(org, refp, blk, s, ss, (-95, -95, 39, 39, 5, 5), mv), oracle_best(org, refp, blk, s, ss, (-4, -4, 9, 9, 1, 1), mv))
    for a in want.values():
        a[0].setflags(write=False), a[1].setflags(write=False)
    return org, refp, ref_xy, mv, want


@pytest.mark.parametrize("wgs", ["8", None])
@pytest.mark.parametrize("ss", [1, 0])
@pytest.mark.parametrize("n16x,n16y,ref_dx", GRIDS)
def test_me_hier_touch_ahead_keeps_the_records(monkeypatch, n16x, n16y, ref_dx, ss, wgs):
    from vvcsoftware_vtm_amd import ops
    if wgs is None:
        monkeypatch.delenv("VVCGPU_MH_WGS", raising=False)
    else:
        monkeypatch.setenv("VVCGPU_MH_WGS", wgs)
    org, refp, ref_xy, mv, want = case(n16x, n16y, ref_dx, ss)
    raster, dense = ops.me_hier_search(dev(org), dev(refp), (0, 0), ref_xy, n16x, n16y, ss, 96, 4, mv)
    torch.cuda.synchronize()
    for k, s in enumerate((16, 32, 64)):
        if s not in want:
            assert raster[k] is None
            continue
        assert np.array_equal(raster[k].cpu().numpy().view(ops.SEARCH_BEST), want[s][0]), "raster %dx%d" % (s, s)
        assert np.array_equal(dense[k].cpu().numpy().view(ops.SEARCH_BEST), want[s][1]), "dense %dx%d" % (s, s)
