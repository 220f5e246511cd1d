"""The matrix-core refinement of 16x16 PUs (frac16m_kernel) on the inputs that reach the ends of its arithmetic and every path of its walk, against the
CPU oracle (orc_frac_refine), Hadamard cost on, planes of at most 320x192:
  * the limbs of the first-stage planes and of the tile sums at their bounds, per bit depth and with both clamps acting;
  * every one of the 9 x 9 (half-sample winner, quarter-sample winner) pairs;
  * both kernel forms (four and sixteen waves per workgroup), flagged PUs and per-PU predictors in a list with a ragged last round;
  * the motion vector cost: ties, the longest exp-Golomb codes 32-bit vectors allow, costs beyond 32 bits, negative vectors."""
import ctypes as C
import numpy as np
import pytest
import torch

import cases
from oraclelib import oracle, p

pytestmark = pytest.mark.gpu

PW, PH, M, N = 320, 192, 16, 16                              # the padded reference plane, its margin, the PU size
W, H = PW - 2 * M, PH - 2 * M                                # the original plane


def dev(a):
    return torch.from_numpy(a).cuda()


def run_both(org, ref, blk, bd, mv, clp):
    """-> (device answers, oracle answers) of one vvcgpu_frac_refine call"""
    from vvcsoftware_vtm_amd import ops
    assert ref.shape == (PH, PW) and org.shape == (H, W) and org.dtype == ref.dtype == np.int16
    lo = np.minimum(blk["ref_x"], blk["org_x"] + M), np.minimum(blk["ref_y"], blk["org_y"] + M)
    hi = np.maximum(blk["ref_x"], blk["org_x"] + M), np.maximum(blk["ref_y"], blk["org_y"] + M)
    assert lo[0].min() >= 8 and lo[1].min() >= 8 and hi[0].max() + N + 8 <= PW and hi[1].max() + N + 8 <= PH      # every window inside the plane
    nb = len(blk)
    want = np.zeros(nb, ops.FRAC_RESULT)
    oracle().orc_frac_refine(p(org), W, p(ref), PW, p(blk), nb, N, N, bd, clp[0], clp[1], 1, C.byref(mv), p(want))
    got = ops.frac_refine(dev(org), dev(ref), ops.struct_to_device(blk), nb, N, N, bd, mv, True, clp).cpu().numpy().view(ops.FRAC_RESULT)
    return got, want


def same(got, want):
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (bad.size, bad[:5], got[bad[:3]], want[bad[:3]])


def blocks_every_phase(rng):
    """16 PUs whose integer vectors take every (x mod 4, y mod 4)"""
    from vvcsoftware_vtm_amd import ops
    rows = []
    for ay in range(4):
        for ax in range(4):
            x, y = int(rng.integers(12, W - N - 12)), int(rng.integers(12, H - N - 12))
            mvx, mvy = 4 * int(rng.integers(-1, 2)) + ax - (4 if ax > 1 else 0), 4 * int(rng.integers(-1, 2)) + ay - (4 if ay > 1 else 0)
            rows.append((x, y, M + x + mvx, M + y + mvy, mvx, mvy))
    blk = np.array(rows, ops.FRAC_BLK)
    assert len({(int(r["mv_x"]) & 3, int(r["mv_y"]) & 3) for r in blk}) == 16
    return blk


REF_KINDS = ("zero", "max", "checker", "rows", "columns", "extreme")
ORG_KINDS = ("zero", "max", "random")


def bound_plane(rng, kind, h, w, bd):
    mx = (1 << bd) - 1
    yy, xx = np.mgrid[0:h, 0:w]
    if kind == "zero":
        return np.zeros((h, w), np.int16)
    if kind == "max":
        return np.full((h, w), mx, np.int16)
    if kind == "checker":
        return (((yy + xx) & 1) * mx).astype(np.int16)
    if kind == "rows":
        return ((yy & 1) * mx).astype(np.int16)
    if kind == "columns":
        return ((xx & 1) * mx).astype(np.int16)
    if kind == "random":
        return cases.rand_plane(rng, h, w, bd, "uniform")
    return cases.rand_plane(rng, h, w, bd, kind)


@pytest.mark.parametrize("narrow", [0, 1])
@pytest.mark.parametrize("bd", [8, 9, 10])
def test_limb_bounds(bd, narrow):
    """Reference windows that put the first-stage planes at both ends of their range (all 0, all maximum, the alternations that meet the taps'
    signs, saturating random content) against originals at 0 / maximum / random, once with the clip range of the bit depth and once with one
    narrowed by 64 at both ends, so that the prediction's lower and upper clamp both act.  The winners of the random patterns are checked to
    take every half-sample offset in x and in y: the quarter stage then walks all seven first-stage and all fourteen second-stage matrices."""
    from vvcsoftware_vtm_amd import ops
    rng = np.random.default_rng(100 * bd + narrow)
    mx = (1 << bd) - 1
    clp = (64, mx - 64) if narrow else (0, mx)
    hxs, hys = set(), set()
    for rk in REF_KINDS:
        ref = bound_plane(rng, rk, PH, PW, bd)
        for ok in ORG_KINDS:
            org = bound_plane(rng, ok, H, W, bd)
            blk = blocks_every_phase(rng)
            mv = ops.MvCost(float(rng.uniform(0.5, 6)), int(rng.integers(-20, 20)), int(rng.integers(-20, 20)), 0, 0)
            got, want = run_both(org, ref, blk, bd, mv, clp)
            same(got, want)
            hxs |= set(want["half_x"].tolist()); hys |= set(want["half_y"].tolist())
    assert hxs == {-1, 0, 1} and hys == {-1, 0, 1}


# sub-sample shifts (in samples) that make (half-sample winner, quarter-sample winner) = (h, q) along one axis: the half stage takes the nearer of
# 0 and +-0.5, the quarter stage the nearest of the three quarter positions around it
SHIFT_OF = {(-1, -1): -0.75, (-1, 0): -0.5, (-1, 1): -0.31, (0, -1): -0.19, (0, 0): 0.0, (0, 1): 0.19, (1, -1): 0.31, (1, 0): 0.5, (1, 1): 0.75}
WINNER_SEED = 3


def winner_case(seed=WINNER_SEED, bd=10):
    """A smooth reference f and an original made of 16x16 tiles, tile t = f shifted by the sub-sample amounts of its target pair: 162 PUs, every
    (half, quarter) target in x crossed with every one in y, twice"""
    from vvcsoftware_vtm_amd import ops
    rng = np.random.default_rng(seed)
    mx = (1 << bd) - 1
    ph = rng.uniform(0, 6.28, 4)

    def f(y, x):
        v = 0.5 + 0.16 * np.sin(x / 3.1 + ph[0]) + 0.16 * np.sin(y / 2.9 + ph[1]) + 0.08 * np.sin((x + y) / 5.3 + ph[2]) + 0.08 * np.sin((x - y) / 4.7 + ph[3])
        return np.clip(np.rint(v * mx), 0, mx).astype(np.int16)

    yy, xx = np.mgrid[0:PH, 0:PW].astype(np.float64)
    ref = f(yy, xx)
    org = np.zeros((H, W), np.int16)
    keys = sorted(SHIFT_OF)
    rows = []
    tiles = [(tx, ty) for ty in range(H // N) for tx in range(W // N)]
    assert len(tiles) >= 2 * 81
    for i in range(2 * 81):
        kx, ky = keys[(i % 81) % 9], keys[(i % 81) // 9]
        tx, ty = tiles[i]
        sign = 1 if i < 81 else -1                             # the second copy mirrored: whichever way the shift's sign maps to the vector's, both occur
        ys, xs = np.mgrid[0:N, 0:N].astype(np.float64)
        org[ty * N:(ty + 1) * N, tx * N:(tx + 1) * N] = f(ys + ty * N + M + sign * SHIFT_OF[ky], xs + tx * N + M + sign * SHIFT_OF[kx])
        rows.append((tx * N, ty * N, M + tx * N, M + ty * N, 0, 0))
    return org, ref, np.array(rows, ops.FRAC_BLK), ops.MvCost(0.01, 0, 0, 0, 0), bd


def test_every_winner():
    """All 81 (half-sample winner, quarter-sample winner) pairs -- 9 x 9 offsets -- occur in the oracle's answers of ONE list, and the device gives
    the same answers: every second-stage plane selection of the quarter stage and every position of the arg-min is taken."""
    org, ref, blk, mv, bd = winner_case()
    got, want = run_both(org, ref, blk, bd, mv, (0, (1 << bd) - 1))
    pairs = {(int(r["half_x"]), int(r["half_y"]), int(r["qter_x"]), int(r["qter_y"])) for r in want}
    assert len(pairs) == 81, sorted(set((hx, hy, qx, qy) for hx in (-1, 0, 1) for hy in (-1, 0, 1) for qx in (-1, 0, 1) for qy in (-1, 0, 1)) - pairs)
    same(got, want)


def random_list(rng, n, bd, ref):
    from vvcsoftware_vtm_amd import ops
    blk = np.zeros(n, ops.FRAC_BLK)
    x, y = rng.integers(12, W - N - 12, n), rng.integers(12, H - N - 12, n)
    mvx, mvy = rng.integers(-3, 4, n), rng.integers(-3, 4, n)
    blk["org_x"], blk["org_y"], blk["ref_x"], blk["ref_y"], blk["mv_x"], blk["mv_y"] = x, y, M + x + mvx, M + y + mvy, mvx, mvy
    return blk


@pytest.mark.parametrize("n", [1, 3, 4, 5, 17])
def test_short_lists_take_the_four_wave_form(n):
    """fewer than 4096 PUs: workgroups of four waves, the last one partly filled (n = 1, 3, 5, 17) or full (4)"""
    from vvcsoftware_vtm_amd import ops
    rng = np.random.default_rng(40 + n)
    bd, mx = 10, 1023
    ref = cases.rand_plane(rng, PH, PW, bd, "smooth")
    org = np.ascontiguousarray(np.clip(ref[M + 1:M + 1 + H, M + 2:M + 2 + W].astype(np.int32) + rng.integers(-6, 7, (H, W)), 0, mx).astype(np.int16))
    got, want = run_both(org, ref, random_list(rng, n, bd, ref), bd, ops.MvCost(5.5, 2, -3, 0, 0), (0, mx))
    same(got, want)


def test_long_list_takes_the_sixteen_wave_form():
    """4096 + 37 PUs through vvcgpu_me_batch (the entry that hands per-PU predictors to the refinement): 256 workgroups of sixteen waves, a second
    round that only 37 waves walk, positions repeating, and about 1 % of the PUs flagged for the vector-pipe body by reference samples outside the
    bit depth in their windows.  The refinement is checked PU by PU, around the integer vector the chain's own search found, with that PU's
    predictor."""
    from vvcsoftware_vtm_amd import ops
    rng = np.random.default_rng(4133)
    bd, mx, n = 10, 1023, 4096 + 37
    org, ref = cases.tz_planes(rng, W, H, M, bd, motion=(2, -1))
    ref = ref.copy()
    wild = [(96, 161), (97, 163)]                               # (row, column) of the padded plane: one below 0, one above the maximum
    ref[wild[0]], ref[wild[1]] = -9, mx + 70
    pus = cases.tz_pus(rng, n, W, H, M, [(N, N)], flags_choices=(0, 1), spread=2)
    pus["org_x"] = np.clip(pus["org_x"], 16, W - N - 16); pus["org_y"] = np.clip(pus["org_y"], 16, H - N - 16)
    pus["pos_x"], pus["pos_y"], pus["ref_x"], pus["ref_y"] = pus["org_x"], pus["org_y"], pus["org_x"] + M, pus["org_y"] + M
    cfg = cases.tz_cfg(W, H, M, 9.5, search_range=4)
    cfg["ref_x0"], cfg["ref_y0"], cfg["ref_x1"], cfg["ref_y1"] = 8, 8, PW - 8, PH - 8      # the search keeps every block 8 samples inside the plane: room for the refinement's taps
    best, frac = ops.me_batch(dev(org), dev(ref), ops.struct_to_device(pus), n, N, N, cfg, bd, use_hadamard=True)
    torch.cuda.synchronize()
    # (the integer stage has its own tests, test_gpu_tzsearch.py; reference samples outside the bit depth are outside what its packed SADs take)
    wb, gf = best.cpu().numpy().view(cases.BEST), frac.cpu().numpy().view(ops.FRAC_RESULT)
    blk = np.zeros(n, ops.FRAC_BLK)
    blk["org_x"], blk["org_y"] = pus["org_x"], pus["org_y"]
    blk["ref_x"], blk["ref_y"] = pus["ref_x"] + wb["x"], pus["ref_y"] + wb["y"]
    blk["mv_x"], blk["mv_y"] = wb["x"], wb["y"]
    assert blk["ref_x"].min() >= 8 and blk["ref_y"].min() >= 8 and blk["ref_x"].max() + N + 8 <= PW and blk["ref_y"].max() + N + 8 <= PH
    O = oracle()
    res = np.zeros(1, ops.FRAC_RESULT)
    nflag = 0
    for i in range(n):
        m = ops.MvCost(9.5, int(pus["pred_hor"][i]), int(pus["pred_ver"][i]), 0, 0)
        O.orc_frac_refine(p(org), W, p(ref), PW, p(blk[i:i + 1]), 1, N, N, bd, 0, mx, 1, C.byref(m), p(res))
        assert gf[i] == res[0], (i, gf[i], res[0])
        nflag += int(any(blk["ref_y"][i] - 4 <= r < blk["ref_y"][i] + 20 and blk["ref_x"][i] - 4 <= c < blk["ref_x"][i] + 20 for r, c in wild))
    assert 20 <= nflag <= 125, nflag                          # about 1 % of 4133
    assert len(set(zip(pus["pred_hor"].tolist(), pus["pred_ver"].tolist()))) > 100


def cost_case(rng, bd, flat):
    mx = (1 << bd) - 1
    if flat:
        return np.full((H, W), 300, np.int16), np.full((PH, PW), 300, np.int16)
    ref = cases.rand_plane(rng, PH, PW, bd, "smooth")
    org = np.ascontiguousarray(np.clip(ref[M:M + H, M + 1:M + 1 + W].astype(np.int32) + rng.integers(-6, 7, (H, W)), 0, mx).astype(np.int16))
    return org, ref


def test_mvcost_ties_take_the_first_index():
    """Flat content: the nine distortions of a stage are equal.  With lambda 0 every cost is equal and the first index -- the centre -- wins both
    stages; with a predictor to one side the cost alone decides."""
    from vvcsoftware_vtm_amd import ops
    rng = np.random.default_rng(11)
    org, ref = cost_case(rng, 10, True)
    blk = random_list(rng, 16, 10, ref)
    got, want = run_both(org, ref, blk, 10, ops.MvCost(0.0, 5, -7, 0, 0), (0, 1023))
    same(got, want)
    assert not want["half_x"].any() and not want["half_y"].any() and not want["qter_x"].any() and not want["qter_y"].any()
    got, want = run_both(org, ref, blk, 10, ops.MvCost(3.0, 3, -3, 0, 0), (0, 1023))
    same(got, want)
    assert want["half_x"].any() and want["half_y"].any() and (want["qter_x"].any() or want["qter_y"].any())


@pytest.mark.parametrize("pred", [(1 << 29, -(1 << 29)), (-(1 << 29) + 3, (1 << 29) - 1), ((1 << 29) + 12345, -(1 << 28))])
def test_mvcost_longest_codes(pred):
    """Predictors 2^29 quarter samples away, as far as the signed 32-bit arithmetic of the cost (2 |d| + 1) goes without wrapping: the exp-Golomb
    argument t then has 31 bits and a length 1 + 2 floorLog2(t) of 61 bits per component, 122 in all.  (A count of 160 bits, the size of the kernel's
    cost table, cannot occur: a 32-bit t gives at most 63 bits per component, 126 in all; the table is therefore read by every candidate and the
    path beyond it taken by none.)"""
    from vvcsoftware_vtm_amd import ops
    rng = np.random.default_rng(12)
    org, ref = cost_case(rng, 10, False)
    got, want = run_both(org, ref, random_list(rng, 16, 10, ref), 10, ops.MvCost(4.25, pred[0], pred[1], 0, 0), (0, 1023))
    same(got, want)


@pytest.mark.parametrize("lam", [3.0e9, 1.0e17])
def test_mvcost_beyond_32_bits(lam):
    """lambda x bits beyond 2^32 (with the second value up to 2^61): the arg-min leaves its 32-bit form for the 64-bit one.  Flat content as well,
    where only the 64-bit costs differ."""
    from vvcsoftware_vtm_amd import ops
    rng = np.random.default_rng(13)
    for flat in (False, True):
        org, ref = cost_case(rng, 10, flat)
        got, want = run_both(org, ref, random_list(rng, 16, 10, ref), 10, ops.MvCost(lam, 9, -14, 0, 0), (0, 1023))
        same(got, want)
        assert int(want["cost"].min()) >> 32


def test_mvcost_negative_vectors():
    """integer vectors and predictors on the negative side, next to zero and far from it"""
    from vvcsoftware_vtm_amd import ops
    rng = np.random.default_rng(14)
    org, ref = cost_case(rng, 10, False)
    blk = random_list(rng, 32, 10, ref)
    blk["mv_x"], blk["mv_y"] = -rng.integers(0, 4, 32), -rng.integers(0, 4, 32)
    blk["ref_x"], blk["ref_y"] = M + blk["org_x"] + blk["mv_x"], M + blk["org_y"] + blk["mv_y"]
    for pred in ((-1, -2), (-4000, -3), (2, -70000)):
        got, want = run_both(org, ref, blk, 10, ops.MvCost(7.0, pred[0], pred[1], 0, 0), (0, 1023))
        same(got, want)
