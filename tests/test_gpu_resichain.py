"""vvcgpu_resi_chain_batch (residual -> T1 -> Quant::quant -> Quant::dequant -> T2 -> reconstruction in one pass) against the oracle's
restatement of the five separate steps (orc_pelop_batch / orc_tr_fwd_batch / orc_quant_batch / orc_dequant_tr_inv_batch / orc_pelop_batch),
each of which is pinned against the compiled reference (tests/test_oracle_golden.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

import cases
from oraclelib import oracle, p
from vvcsoftware_vtm_amd.abi import DQTR_DESC, PELOP_DESC, QUANT_DESC, TR_DESC, PelopCfg

pytestmark = pytest.mark.gpu


def oracle_chain(org, pred, tus, bd, W):
    """tus: list of (x, y, w, h, tr_hor, tr_ver, qp, intra, sbh) -> (levels, abs_sum, rec)"""
    H = org.shape[0]
    mx = (1 << bd) - 1
    n = len(tus)
    tr = np.zeros(n, TR_DESC); qd = np.zeros(n, QUANT_DESC); dq = np.zeros(n, DQTR_DESC); bands = np.zeros(n, PELOP_DESC)
    coff = 0
    for i, (x, y, w, h, th, tv, qp, intra, sbh) in enumerate(tus):
        tr[i] = (y * W + x, coff, W, w, h, th, tv, 0, 0)
        qd[i] = (coff, coff, w, h, intra, sbh, 0, qp, 0)
        dq[i] = (y * W + x, coff, W, w, h, th, tv, 0, 0, qp)
        bands[i] = (y * W + x, y * W + x, y * W + x, W, W, W, w, h)
        coff += w * h
    resi = np.zeros((H, W), np.int16); resi2 = np.zeros((H, W), np.int16)
    coef = np.zeros(coff, np.int32); level = np.zeros(coff, np.int32); dqc = np.zeros(coff, np.int32); abs_sum = np.zeros(n, np.uint32)
    rec = pred.copy()
    o = oracle()
    o.orc_pelop_batch(3, p(org), p(pred), p(resi), p(bands), n, C.byref(PelopCfg(0, 0, 0, 0, 0, mx)))
    o.orc_tr_fwd_batch(p(resi), p(coef), p(tr), n, bd)
    o.orc_quant_batch(p(coef), p(level), p(qd), n, bd, p(abs_sum))
    o.orc_dequant_tr_inv_batch(p(level), p(resi2), p(dq), n, bd, p(dqc))
    o.orc_pelop_batch(1, p(pred), p(resi2), p(rec), p(bands), n, C.byref(PelopCfg(0, 0, 0, 1, 0, mx)))
    return level, abs_sum, rec, tr["coeff_off"].copy()


def gpu_chain(org, pred, tus, bd, W, coffs):
    from vvcsoftware_vtm_amd import ops
    n = len(tus)
    d = np.zeros(n, ops.RC_DESC)
    for i, (x, y, w, h, th, tv, qp, intra, sbh) in enumerate(tus):
        d[i] = (y * W + x, y * W + x, y * W + x, coffs[i], W, W, W, w, h, th, tv, intra, sbh, qp, (0, 0))
    total = int(sum(t[2] * t[3] for t in tus))
    dorg, dpred = torch.from_numpy(org).cuda(), torch.from_numpy(pred).cuda()
    drec = dpred.clone()
    dlevel = torch.full((total,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    a = ops.resi_chain_batch(dorg, dpred, drec, dlevel, ops.struct_to_device(d), n, bd, (0, (1 << bd) - 1))
    torch.cuda.synchronize()
    return dlevel.cpu().numpy(), a.cpu().numpy().view(np.uint32), drec.cpu().numpy()


def runs_of(tus):
    """(w, h, count) of a list grouped by shape"""
    runs = []
    for t in tus:
        if runs and runs[-1][0] == t[2] and runs[-1][1] == t[3]:
            runs[-1][2] += 1
        else:
            runs.append([t[2], t[3], 1])
    return runs


def gpu_chain_runs(org, pred, tus, runs, bd, W, coffs):
    """vvcgpu_resi_chain_runs_batch on a list grouped by shape"""
    from vvcsoftware_vtm_amd import ops
    n = len(tus)
    d = np.zeros(n, ops.RC_DESC)
    for i, (x, y, w, h, th, tv, qp, intra, sbh) in enumerate(tus):
        d[i] = (y * W + x, y * W + x, y * W + x, coffs[i], W, W, W, w, h, th, tv, intra, sbh, qp, (0, 0))
    dorg, dpred = torch.from_numpy(org).cuda(), torch.from_numpy(pred).cuda()
    drec = dpred.clone()
    dlevel = torch.full((int(sum(t[2] * t[3] for t in tus)),), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    a = ops.resi_chain_runs_batch(dorg, dpred, drec, dlevel, ops.struct_to_device(d), n, runs, bd, (0, (1 << bd) - 1))
    torch.cuda.synchronize()
    return dlevel.cpu().numpy(), a.cpu().numpy().view(np.uint32), drec.cpu().numpy()


def tile(W, H, shapes, rng, qps, bd, types_small=True):
    """non-overlapping TUs: the plane is cut into 64x64 cells, each cell tiled with one shape"""
    tus = []
    ci = 0
    for y0 in range(0, H, 64):
        for x0 in range(0, W, 64):
            w, h = shapes[ci % len(shapes)]
            ci += 1
            for ty in range(0, 64, h):
                for tx in range(0, 64, w):
                    th = int(rng.integers(0, 3)) if w <= 32 and w >= 4 else 0
                    tv = int(rng.integers(0, 3)) if h <= 32 and h >= 4 else 0
                    tus.append((x0 + tx, y0 + ty, w, h, th, tv, int(rng.choice(qps)) + 6 * (bd - 8), int(rng.integers(0, 2)), int(rng.integers(0, 4) != 0)))
    return tus


@pytest.mark.parametrize("bd,content", [(10, "smooth"), (10, "uniform"), (8, "smooth"), (10, "extreme")])
def test_resi_chain_squares(bd, content):
    """the shapes of the canonical workload (64 ... 4 squared, every transform pair, QP 22..37, sign hiding on / off, both slice types)"""
    rng = np.random.default_rng(bd * 5 + len(content))
    W, H = 448, 192
    org = cases.rand_plane(rng, H, W, bd, content)
    pred = cases.rand_plane(rng, H, W, bd, "smooth" if content != "extreme" else "extreme")
    if content == "smooth":                      # small residual: many zero levels, sparse coefficient groups (last-group logic)
        pred = np.clip(org + rng.integers(-6, 7, org.shape), 0, (1 << bd) - 1).astype(np.int16)
    tus = tile(W, H, [(64, 64), (32, 32), (16, 16), (8, 8), (4, 4)], rng, [22, 27, 32, 37, 45], bd)
    lv, asum, rec, coffs = oracle_chain(org, pred, tus, bd, W)
    glv, gsum, grec = gpu_chain(org, pred, tus, bd, W, coffs)
    assert np.array_equal(gsum, asum)
    assert np.array_equal(glv, lv)
    assert np.array_equal(grec, rec)


@pytest.mark.parametrize("W,H,shapes,per_wave", [(1536, 1024, [(4, 4), (16, 16), (4, 4), (16, 16), (32, 32)], 1),
                                                 (2048, 1024, [(4, 4), (4, 4), (4, 4), (16, 16)], 2),
                                                 (2048, 1024, [(8, 8), (8, 8), (16, 16)], 8),
                                                 (2560, 1024, [(4, 4), (4, 4), (4, 4), (16, 16)], 2)])
def test_resi_chain_prologue_items(W, H, shapes, per_wave):
    """lists long enough for the chain launch's prologue (one wave of a workgroup copies the matrix image, the other three run one / two items of the
    4x4 class -- or one of the 8x8 class -- taken from the end of that class's list): every TU served exactly once, results as the oracle's"""
    rng = np.random.default_rng(W + per_wave)
    bd = 10
    org = cases.rand_plane(rng, H, W, bd, "smooth")
    pred = np.clip(org + rng.integers(-25, 26, org.shape), 0, 1023).astype(np.int16)
    tus = tile(W, H, shapes, rng, [22, 32, 37], bd)
    items4 = (sum(1 for t in tus if t[2] == 4 and t[3] == 4) + 15) // 16
    items8 = (sum(1 for t in tus if t[2] == 8 and t[3] == 8) + 7) // 8
    if per_wave == 8:                                                              # no 4x4 TUs: one 8x8 item per wave
        assert items4 == 0 and items8 >= 3 * 768
    else:
        assert (items4 >= 6 * 768) == (per_wave == 2) and items4 >= 3 * 768      # (768 workgroups: the launch's grid)
    lv, asum, rec, coffs = oracle_chain(org, pred, tus, bd, W)
    glv, gsum, grec = gpu_chain(org, pred, tus, bd, W, coffs)
    assert np.array_equal(gsum, asum)
    assert np.array_equal(glv, lv)
    assert np.array_equal(grec, rec)


def test_resi_chain_rectangles_and_chroma_shapes():
    """every other W x H in 2..64 takes the generic path: rectangles with 2:1 ... 16:1 aspect, 2-wide chroma TUs"""
    rng = np.random.default_rng(77)
    bd, W, H = 10, 512, 128
    org = cases.rand_plane(rng, H, W, bd, "smooth")
    pred = np.clip(org + rng.integers(-40, 41, org.shape), 0, 1023).astype(np.int16)
    shapes = [(64, 32), (32, 64), (16, 32), (32, 16), (64, 16), (8, 16), (16, 8), (4, 16), (4, 64), (64, 4), (16, 4), (4, 8), (8, 4), (2, 8), (8, 2), (2, 2), (16, 64), (32, 8), (2, 32)]
    tus = tile(W, H, shapes, rng, [27, 32, 37, 22, 24, 29], bd)                 # every qp % 6
    lv, asum, rec, coffs = oracle_chain(org, pred, tus, bd, W)
    glv, gsum, grec = gpu_chain(org, pred, tus, bd, W, coffs)
    assert np.array_equal(gsum, asum)
    assert np.array_equal(glv, lv)
    assert np.array_equal(grec, rec)


@pytest.mark.parametrize("bd,content", [(10, "smooth"), (8, "smooth"), (10, "extreme"), (10, "uniform")])
def test_resi_chain_packed_tiles(bd, content):
    """16x8 / 8x16 / 16x4 / 4x16 (and 32x8 .. 4x32, 64x8 .. 4x64 in multi-tiles, the 64-point side with its zero-out): two or four TUs share one 16x16 matrix-core tile (rc_tile_packed*),
    every TU with its own transform pair, QP, slice type
    and sign-hiding flag; class counts that leave the last tile part-filled; a few TUs whose residual leaves +-1023 sit in tiles with ordinary
    ones and must reach the generic path alone"""
    rng = np.random.default_rng(bd * 11 + len(content))
    W, H = 896, 128
    org = cases.rand_plane(rng, H, W, bd, content)
    pred = cases.rand_plane(rng, H, W, bd, "smooth" if content != "extreme" else "extreme")
    if content == "smooth":
        pred = np.clip(org + rng.integers(-9, 10, org.shape), 0, (1 << bd) - 1).astype(np.int16)
    tus = tile(W, H, [(16, 8), (8, 16), (16, 4), (4, 16), (16, 16), (8, 8), (32, 8), (8, 32), (32, 4), (4, 32), (64, 8), (8, 64), (64, 4), (4, 64)], rng, [22, 27, 30, 32, 35, 37, 45], bd)   # every qp % 6
    keep = rng.random(len(tus)) > 0.07                       # odd counts per class, tiles whose TUs are not neighbours in the picture
    tus = [t for t, k in zip(tus, keep) if k]
    order = rng.permutation(len(tus))
    tus = [tus[i] for i in order]
    if content == "smooth" and bd == 10:
        org = org.copy()
        for i in rng.choice(len(tus), 25, replace=False):    # out of the matrix-core range: |org - pred| > 1023
            x, y, w, h = tus[i][:4]
            org[y + int(rng.integers(0, h)), x + int(rng.integers(0, w))] = -2500
    lv, asum, rec, coffs = oracle_chain(org, pred, tus, bd, W)
    glv, gsum, grec = gpu_chain(org, pred, tus, bd, W, coffs)
    assert np.array_equal(gsum, asum), np.nonzero(gsum != asum)[0][:8]
    assert np.array_equal(glv, lv)
    assert np.array_equal(grec, rec)


def test_resi_chain_residual_outside_range_falls_back():
    """samples outside the bit depth (|residual| > 1023) leave the matrix-core path's exactness range: those TUs are served by the generic path"""
    rng = np.random.default_rng(5)
    bd, W, H = 10, 192, 64
    org = rng.integers(-3000, 3000, (H, W)).astype(np.int16)
    pred = rng.integers(0, 1024, (H, W)).astype(np.int16)
    tus = tile(W, H, [(64, 64), (32, 32), (16, 16)], rng, [32], bd)
    lv, asum, rec, coffs = oracle_chain(org, pred, tus, bd, W)
    glv, gsum, grec = gpu_chain(org, pred, tus, bd, W, coffs)
    assert np.array_equal(gsum, asum) and np.array_equal(glv, lv) and np.array_equal(grec, rec)


def test_resi_chain_rejects_transform_skip_descriptor():
    from vvcsoftware_vtm_amd import ops
    bd, W, H = 10, 64, 64
    org = np.full((H, W), 500, np.int16)
    tus = [(0, 0, 4, 4, 3, 0, 32 + 12, 0, 1), (8, 0, 4, 4, 0, 0, 32 + 12, 0, 1)]
    d = np.zeros(2, ops.RC_DESC)
    for i, (x, y, w, h, th, tv, qp, intra, sbh) in enumerate(tus):
        d[i] = (y * W + x, y * W + x, y * W + x, 16 * i, W, W, W, w, h, th, tv, intra, sbh, qp, (0, 0))
    t = torch.from_numpy(org).cuda()
    rec = t.clone()
    lvl = torch.zeros(32, dtype=torch.int32, device="cuda")
    a = ops.resi_chain_batch(t, t.clone(), rec, lvl, ops.struct_to_device(d), 2, bd).cpu().numpy().view(np.uint32)
    assert a[0] == 0xFFFFFFFF and a[1] == 0


def test_stream_counters_survive_interleaved_entry_points():
    """vvcgpu_resi_chain_batch and vvcgpu_mc_batch take their zeroed work counters from the stream's persistent pair (lib.hip: vvcgpu_counters) and
    each call clears the other set for the next one.  Calls of both kinds in every order, with lists that leave different counts behind
    (a chain with TUs of every class and fall-back TUs, then one with a single class; MC lists with and without PUs for the generic kernel),
    must all give the oracle's results."""
    from vvcsoftware_vtm_amd import ops
    rng = np.random.default_rng(4242)
    bd, W, H = 10, 256, 128
    mx = (1 << bd) - 1
    org = cases.rand_plane(rng, H, W, bd, "uniform")
    pred = np.clip(org + rng.integers(-30, 31, org.shape), 0, mx).astype(np.int16)
    wild = rng.integers(-3000, 3000, (H, W)).astype(np.int16)                       # |residual| > 1023: fall-back list of the chain
    tus_all = tile(W, H, [(64, 64), (32, 32), (16, 16), (8, 8), (4, 4), (16, 8)], rng, [27, 37], bd)
    tus_one = tile(W, H, [(8, 8)], rng, [32], bd)
    want = {}
    for name, (o_, tus) in {"all": (org, tus_all), "one": (org, tus_one), "wild": (wild, tus_all)}.items():
        want[name] = oracle_chain(o_, pred, tus, bd, W)

    # MC lists: ref = a padded plane, 16x16 luma PUs (fast kernel) with and without a few 32x8 PUs (generic kernel)
    M = 16
    ref = np.ascontiguousarray(np.pad(cases.rand_plane(rng, H, W, bd, "smooth"), M, mode="edge"))
    RS = W + 2 * M

    def mc_list(extra):
        rows, dst_off = [], 0
        for y in range(0, H, 16):
            for x in range(0, W // 2, 16):
                rows.append(((y + M) * RS + x + M + int(rng.integers(-3, 4)), 0, dst_off, RS, RS, 16, 16, 16, int(rng.integers(0, 4)), int(rng.integers(0, 4)), 0, 0, 1, 0, 0))
                dst_off += 256
        for k in range(extra):
            rows.append(((M + 8 * k) * RS + M + 64, 0, dst_off, RS, RS, 32, 32, 8, 1 + k % 3, 2, 0, 0, 1, 0, 0))
            dst_off += 256
        d = np.zeros(len(rows), ops.MC_DESC)
        for i, r in enumerate(rows):
            d[i] = r
        return d, dst_off

    def mc_oracle(d, total):
        out = np.zeros(total, np.int16)
        oracle().orc_mc_batch(p(ref), p(ref), p(out), p(d), d.size, bd, 0, mx)
        return out

    mc = {k: mc_list(e) for k, e in (("fast", 0), ("mixed", 5))}
    mc_want = {k: mc_oracle(*v) for k, v in mc.items()}
    dref = torch.from_numpy(ref).cuda()

    def run_chain(name):
        o_, tus = {"all": (org, tus_all), "one": (org, tus_one), "wild": (wild, tus_all)}[name]
        lv, asum, rec, coffs = want[name]
        glv, gsum, grec = gpu_chain(o_, pred, tus, bd, W, coffs)
        assert np.array_equal(gsum, asum) and np.array_equal(glv, lv) and np.array_equal(grec, rec), name

    def run_mc(name):
        d, total = mc[name]
        dst = torch.zeros(total, dtype=torch.int16, device="cuda")
        ops.mc_batch(dref, dref, dst, ops.struct_to_device(d), d.size, bd, (0, mx))
        assert np.array_equal(dst.cpu().numpy(), mc_want[name]), name

    for step in ["all", "mixed", "one", "wild", "wild", "fast", "mixed", "mixed", "all", "one", "fast", "all"]:
        (run_mc if step in mc else run_chain)(step)


@pytest.mark.parametrize("bd,content", [(10, "smooth"), (8, "uniform")])
def test_resi_chain_runs_entry_equals_the_classified_entry(bd, content):
    """vvcgpu_resi_chain_runs_batch: descriptors grouped by shape, runs (w, h, count) from the host -- no classification launch.  Every shape the chain
    has a body for (squares, rectangles, packed tiles), in an order of the caller's choosing, a few TUs outside the matrix-core range (fall-back list), twice on
    one stream with different lists (the identity array and the counter sets persist); equal to the oracle, i.e. to vvcgpu_resi_chain_batch.  A list
    that holds a 2-wide shape is served through the classified path."""
    from vvcsoftware_vtm_amd import ops
    rng = np.random.default_rng(bd * 3 + len(content))
    W, H = 768, 192
    org = cases.rand_plane(rng, H, W, bd, content)
    pred = np.clip(org + rng.integers(-25, 26, org.shape), 0, (1 << bd) - 1).astype(np.int16)
    shapes_all = [(8, 8), (64, 64), (4, 4), (32, 32), (16, 16), (64, 32), (32, 64), (16, 8), (8, 16), (4, 8), (8, 4), (32, 8), (4, 32), (64, 16), (16, 64), (32, 16), (16, 32), (64, 4), (8, 64)]
    for rnd, shapes in enumerate([shapes_all, shapes_all[3:9], shapes_all + [(2, 8)]]):
        tus = tile(W, H, shapes, rng, [22, 32, 37], bd)
        keep = rng.random(len(tus)) > 0.1
        tus = [t for t, k in zip(tus, keep) if k]
        order = sorted(range(len(tus)), key=lambda i: shapes.index((tus[i][2], tus[i][3])))      # grouped by shape, groups in the caller's order
        tus = [tus[i] for i in order]
        runs = runs_of(tus)
        o2 = org.copy()
        if rnd == 0 and bd == 10:
            for i in rng.choice(len(tus), 9, replace=False):
                x, y = tus[i][:2]
                o2[y, x] = -2500
        lv, asum, rec, coffs = oracle_chain(o2, pred, tus, bd, W)
        glv, gsum, grec = gpu_chain_runs(o2, pred, tus, runs, bd, W, coffs)
        assert np.array_equal(gsum, asum), rnd
        assert np.array_equal(glv, lv), rnd
        assert np.array_equal(grec, rec), rnd


def test_resi_chain_runs_entry_rejects_inconsistent_runs():
    from vvcsoftware_vtm_amd import ops, capi
    t = torch.zeros((64, 64), dtype=torch.int16, device="cuda")
    lvl = torch.zeros(4096, dtype=torch.int32, device="cuda")
    d = np.zeros(4, ops.RC_DESC)
    d["w"] = d["h"] = 8
    dd = ops.struct_to_device(d)
    for runs in ([(8, 8, 3)], [(8, 8, 2), (8, 8, 2)], [(8, 3, 4)]):
        with pytest.raises(capi.VvcGpuError):
            ops.resi_chain_runs_batch(t, t, t.clone(), lvl, dd, 4, runs, 10)


def assert_chain(got, want, tus, coffs):
    """levels, abs_sum and reconstruction equal; on a mismatch the message names the TUs"""
    (glv, gsum, grec), (lv, asum, rec) = got, want
    bad = [t for i, t in enumerate(tus) if gsum[i] != asum[i] or not np.array_equal(glv[coffs[i]:coffs[i] + t[2] * t[3]], lv[coffs[i]:coffs[i] + t[2] * t[3]])
           or not np.array_equal(grec[t[1]:t[1] + t[3], t[0]:t[0] + t[2]], rec[t[1]:t[1] + t[3], t[0]:t[0] + t[2]])]
    assert not bad, (len(bad), bad[:8])
    assert np.array_equal(gsum, asum) and np.array_equal(glv, lv) and np.array_equal(grec, rec)


@pytest.mark.parametrize("bd", [8, 10])
def test_resi_chain_at_the_exactness_bound(bd):
    """cases.chain_bound_case: residuals of +-max whose signs follow a basis row, all 29 shapes (co-operative 64 / 32 forms, one-wave matrix-core
    rectangles, the 16x16 walk, packed tiles, lane groups, the generic launch for the 2-wide ones), QP 0 .. 22 + 6 (bd - 8): first-stage sums of
    16 760 832 of 2^24 (bit depth 10), limbs at hi = 128, levels clipped to +-32767 / -32768 by the quantiser while abs_sum keeps the unclipped magnitudes,
    the sign-hiding special case of a level on the clip, the de-quantiser's clip.  Through the classified entry, then (without the shapes with a 2-point side,
    which make that entry take the classified path) grouped by shape through the runs entry."""
    org, pred, tus, W = cases.chain_bound_case(bd)
    lv, asum, rec, coffs = oracle_chain(org, pred, tus, bd, W)
    assert_chain(gpu_chain(org, pred, tus, bd, W, coffs), (lv, asum, rec), tus, coffs)
    shapes = sorted({(t[2], t[3]) for t in tus if min(t[2], t[3]) >= 4})
    grouped = sorted((t for t in tus if min(t[2], t[3]) >= 4), key=lambda t: shapes.index((t[2], t[3])))
    assert len(shapes) == 25
    lv, asum, rec, coffs = oracle_chain(org, pred, grouped, bd, W)
    assert_chain(gpu_chain_runs(org, pred, grouped, runs_of(grouped), bd, W, coffs), (lv, asum, rec), grouped, coffs)


def threshold_case(rng, bd=10):
    """quiet TUs (|org - pred| <= 20), every third (packed tiles, lane groups: TUs that share a tile) or second one with ONE sample whose residual is
    +-1023 (the last value the matrix-core bodies take), +-1024 (the first they hand over; still an exact f16 value: it shows a TU lost or served twice) or
    16392 / -16408 (no f16 values, 8 away from the next one: a TU that a missed vote keeps on the matrix cores gets different levels), org outside the bit depth where that needs it:
    -> org, pred, tus, W, indices of the touched TUs"""
    mx = (1 << bd) - 1
    single = [(64, 64), (64, 32), (32, 64), (32, 32), (64, 16), (16, 64), (32, 16), (16, 32), (16, 16)]
    shared = [(16, 8), (8, 16), (16, 4), (4, 16), (32, 8), (8, 32), (32, 4), (4, 32), (64, 8), (8, 64), (64, 4), (4, 64), (8, 8), (4, 4), (8, 4), (4, 8)]
    want = []                                                # (w, h, None | (x, y, v))
    for (w, h) in single + shared:
        pts = [(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1), (w // 2 - 1, h // 2), (w - 1, h // 2)]
        pts += [(min(w // 2 + 3, w - 1), 16 * s_ + 5) for s_ in range(h // 16)] if h >= 32 else []      # a sample in every wave's row strip of the co-operative form
        for pt in pts:
            for v in (1023, -1023, 1024, -1024, 16392, -16408):
                want += [(w, h, pt + (v,))] + [(w, h, None)] * (1 if (w, h) in single else 2)
    want += [(16, 16, (i % 16, (i // 16) % 16, (1024, -1024, 1023, 16392, -16408)[i % 5]) if i % 53 == 0 else None) for i in range(3200)]   # > 4 x 768: the 16x16 walk goes round
    by_shape = {}
    for i, (w, h, t) in enumerate(want):
        by_shape.setdefault((w, h), []).append(i)
    W = 1024
    pos = {}
    cell = 0
    for (w, h), idx in by_shape.items():                     # 64 x 64 cells, one shape per cell
        per = (64 // w) * (64 // h)
        for j, i in enumerate(idx):
            c = cell + j // per
            q = j % per
            pos[i] = ((c % 16) * 64 + (q % (64 // w)) * w, (c // 16) * 64 + (q // (64 // w)) * h)
        cell += (len(idx) + per - 1) // per
    H = ((cell + 15) // 16) * 64
    pred = rng.integers(100, mx - 100, (H, W)).astype(np.int16)
    org = (pred + rng.integers(-20, 21, (H, W))).astype(np.int16)
    tus, touched = [], []
    for i, (w, h, t) in enumerate(want):
        x0, y0 = pos[i]
        if t is not None:
            x, y, v = t
            org[y0 + y, x0 + x], pred[y0 + y, x0 + x] = {1023: (mx, 0), -1023: (0, mx), 1024: (mx + 1, 0), -1024: (-1, mx), 16392: (16392, 0), -16408: (mx - 16408, mx)}[v]
            touched.append(i)
        th = int(rng.integers(0, 3)) if 4 <= w <= 32 else 0
        tv = int(rng.integers(0, 3)) if 4 <= h <= 32 else 0
        tus.append((x0, y0, w, h, th, tv, (4, 22, 0)[i % 3] + 6 * (bd - 8), i & 1, (i >> 1) & 1))
    return org, pred, tus, W, touched


def test_resi_chain_single_sample_across_the_threshold():
    """the range vote of every matrix-core class (co-operative 64 / 32 forms: the flag one wave raises must stop all four; one-wave rectangles; the
    16x16 walk with more than 4 x 768 TUs, so that it goes round and sets TUs aside), of every packed-tile class and of the lane groups, with the
    sample on the limit (+-1023: stays) and one past it (+-1024: handed to the generic body on the spot) at lanes of every kind.  The quiet TUs that share a
    tile, a lane group or a slot with such a TU keep their fast path's results."""
    rng = np.random.default_rng(1024)
    org, pred, tus, W, touched = threshold_case(rng)
    assert len(touched) > 1100 and sum(1 for t in tus if t[2:4] == (16, 16)) > 4 * 768
    lv, asum, rec, coffs = oracle_chain(org, pred, tus, 10, W)
    assert_chain(gpu_chain(org, pred, tus, 10, W, coffs), (lv, asum, rec), tus, coffs)
