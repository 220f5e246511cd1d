"""GPU: empty batches, error behaviour and ragged / minimal pictures through the C ABI (the reference's own behaviour for these
cases: an empty loop does nothing; unsupported configurations are rejected up front instead of silently mis-computed)."""
import ctypes as C
import numpy as np
import pytest
import torch

import cases
from oraclelib import oracle, p

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(a).cuda()


def test_empty_batches_leave_outputs_untouched():
    from vvcsoftware_vtm_amd import ops
    plane = torch.full((64, 64), 7, dtype=torch.int16, device="cuda")
    out16 = torch.full((64 * 64,), 9, dtype=torch.int16, device="cuda")
    out32 = torch.full((64 * 64,), 9, dtype=torch.int32, device="cuda")
    dummy = torch.zeros(64, dtype=torch.uint8, device="cuda")
    assert ops.dist_batch(0, plane, plane, dummy, 0).numel() == 0
    ops.if_batch(plane, out16, dummy, 0)
    ops.mc_batch(plane, plane, out16, dummy, 0)
    ops.pelop_batch(1, plane, plane, out16, dummy, 0, ops.PelopCfg(0, 0, 0, 1, 0, 1023))
    ops.tr_fwd_batch(plane, out32, dummy, 0)
    ops.tr_inv_batch(out32, out16, dummy, 0)
    sad, best = ops.sad_search(plane, plane, dummy, 0, 16, 16, 0, -1, -1, 3, 3, 1, 1, ops.MvCost(1.0, 0, 0, 2, 0))
    assert sad.shape[0] == 0
    assert ops.frac_refine(plane, plane, dummy, 0, 16, 16, 10, ops.MvCost(1.0, 0, 0, 0, 0)).numel() == 0
    torch.cuda.synchronize()
    assert bool((out16 == 9).all()) and bool((out32 == 9).all())


def test_rejected_arguments_carry_a_message():
    from vvcsoftware_vtm_amd import ops, capi
    plane = torch.zeros((64, 64), dtype=torch.int16, device="cuda")
    out32 = torch.zeros(64 * 64, dtype=torch.int32, device="cuda")
    blk = ops.struct_to_device(np.array([(8, 8, 8, 8)], ops.SEARCH_BLK))
    mv = ops.MvCost(1.0, 0, 0, 2, 0)
    with pytest.raises(capi.VvcGpuError, match="unsupported"):          # odd block width
        ops.sad_search(plane, plane, blk, 1, 7, 8, 0, -1, -1, 3, 3, 1, 1, mv)
    with pytest.raises(capi.VvcGpuError, match="sub_shift"):
        ops.sad_search(plane, plane, blk, 1, 8, 12, 3, -1, -1, 3, 3, 1, 1, mv)    # 12 rows are not a multiple of 8
    d = np.zeros(1, ops.TR_DESC)
    d[0] = (0, 0, 64, 8, 8, 0, 0, 0, 0)
    with pytest.raises(capi.VvcGpuError, match="bit depth"):
        ops.tr_fwd_batch(plane, out32, ops.struct_to_device(d), 1, 12)
    with pytest.raises(capi.VvcGpuError, match="src must not alias dst"):
        ops.sao_apply(plane, plane, 64, 64, 10, ops.sao_params_to_device(np.zeros(1, ops.SAO_DTYPE)))
    with pytest.raises(capi.VvcGpuError, match="kind"):
        ops.dist_batch(7, plane, plane, torch.zeros(32, dtype=torch.uint8, device="cuda"), 1)


@pytest.mark.parametrize("w,h", [(8, 4), (16, 8), (136, 72), (200, 120), (264, 136)])
def test_inloop_chain_on_ragged_pictures(w, h):
    """pictures that are not a multiple of the CTU (and smaller than one CTU): SAO apply + ALF classify / filter vs the oracle."""
    from vvcsoftware_vtm_amd import ops
    rng = np.random.default_rng(w * 7 + h)
    bd, mx, ctu = 10, 1023, 128
    src = cases.rand_plane(rng, h, w, bd, "smooth")
    prm = cases.sao_params(rng, w, h, ctu, ctu, True)
    want = src.copy()                               # the reference offsets a copy of the deblocked picture
    oracle().orc_sao_apply(p(src), w, p(want), w, w, h, ctu, ctu, bd, p(prm), 0, mx)
    got = torch.zeros((h, w), dtype=torch.int16, device="cuda")
    ops.sao_apply(dev(src), got, ctu, ctu, bd, ops.sao_params_to_device(prm), (0, mx))
    assert np.array_equal(got.cpu().numpy(), want)
    if w % 4 == 0 and h % 4 == 0:
        cls = ops.alf_classify(dev(src), bd).cpu().numpy()
        wcls = np.zeros((h // 4, w // 4), np.uint16)
        oracle().orc_alf_classify(p(src), w, w, h, bd, p(wcls))
        assert np.array_equal(cls.reshape(wcls.shape), wcls)


def test_many_short_lived_streams():
    """A host that creates a stream per job: 100 streams come and go, each running calls that use the library's per-stream resources
    (work lists + persistent counters of vvcgpu_mc_batch, packed blocks of the raster search), released with vvcgpu_stream_release before
    the stream is destroyed.  The 65th stream used to fail for good (fixed table of 64 slots, never reclaimed)."""
    from vvcsoftware_vtm_amd import ops, capi
    rng = np.random.default_rng(5)
    bd, mx, M = 10, 1023, 16
    W, H = 64, 48
    ref = dev(np.ascontiguousarray(np.pad(cases.rand_plane(rng, H, W, bd, "smooth"), M, mode="edge")))
    n = (W // 16) * (H // 16)
    d = np.zeros(n, ops.MC_DESC)
    gx, gy = np.meshgrid(np.arange(0, W, 16), np.arange(0, H, 16))
    d["ref0_off"] = d["ref1_off"] = ((gy.reshape(-1) + M) * (W + 2 * M) + gx.reshape(-1) + M)
    d["dst_off"] = gy.reshape(-1) * W + gx.reshape(-1)
    d["ref0_stride"] = d["ref1_stride"] = W + 2 * M
    d["dst_stride"], d["w"], d["h"], d["is_luma"], d["bi"] = W, 16, 16, 1, 1
    d["frac_x0"], d["frac_y1"] = 4, 8
    dd = ops.struct_to_device(d)
    want = None
    for i in range(100):
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            out = torch.zeros((H, W), dtype=torch.int16, device="cuda")
            ops.mc_batch(ref, ref, out, dd, n, bd, (0, mx))
            s.synchronize()
            got = out.cpu().numpy()
            if want is None:
                want = got
            assert np.array_equal(got, want), i
            capi.call("vvcgpu_stream_release", C.c_void_p(s.cuda_stream))
        del s
    capi.call("vvcgpu_shutdown")
    out = torch.zeros((H, W), dtype=torch.int16, device="cuda")           # the library keeps working after a shutdown (resources come back on demand)
    ops.mc_batch(ref, ref, out, dd, n, bd, (0, mx))
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), want)


def test_me_batch_scratch_grows_inside_the_chain():
    """vvcgpu_me_batch claims the TZ search's and the refinement's workspace from ONE scratch scope.  On one fresh stream: a small call, then a large
    one -- its first claims fit the stream's buffer, a later claim moves the stream to a larger buffer while the earlier claims stay in use (the
    outgrown buffer is retired when the call ends) -- then a small one again.  Each equals the same call on a stream of its own."""
    from vvcsoftware_vtm_amd import ops, capi
    rng = np.random.default_rng(77)
    W, H, M, bd, w, h = 512, 320, 160, 10, 16, 16
    org, ref_ = cases.tz_planes(rng, W, H, M, bd, motion=(3, 2))
    cfg = cases.tz_cfg(W, H, M, 9.5, search_range=32)
    dorg, dref = dev(org), dev(ref_)
    lists = [cases.tz_pus(rng, n, W, H, M, [(w, h)], flags_choices=(0, 1), spread=8) for n in (64, 6000, 100)]
    torch.cuda.synchronize()

    def run(pus, s):
        with torch.cuda.stream(s):
            best, frac = ops.me_batch(dorg, dref, ops.struct_to_device(pus), len(pus), w, h, cfg, bd, use_hadamard=True)
            s.synchronize()
            return best.cpu().numpy(), frac.cpu().numpy()

    shared = torch.cuda.Stream()
    got = [run(pus, shared) for pus in lists]
    capi.call("vvcgpu_stream_release", C.c_void_p(shared.cuda_stream))
    for pus, (gb, gf) in zip(lists, got):
        own = torch.cuda.Stream()
        wb, wf = run(pus, own)
        capi.call("vvcgpu_stream_release", C.c_void_p(own.cuda_stream))
        assert np.array_equal(gb, wb) and np.array_equal(gf, wf), len(pus)


def test_table_images_come_back_after_shutdown():
    """vvcgpu_shutdown releases the per-device table images as well; every user builds its image again on demand: the matrix-core motion
    compensation, the fractional refinement, the forward transform of a long list (chain launch: f16 image + golden tables) and the residual chain
    of shape runs give the same results as before the shutdown."""
    from vvcsoftware_vtm_amd import ops, capi
    rng = np.random.default_rng(11)
    bd, mx, M = 10, 1023, 16
    W, H = 256, 128
    ref = cases.rand_plane(rng, H + 2 * M, W + 2 * M, bd, "smooth")
    org = np.ascontiguousarray(np.clip(ref[M + 1:M + 1 + H, M + 2:M + 2 + W].astype(np.int32) + rng.integers(-6, 7, (H, W)), 0, mx).astype(np.int16))
    dref, dorg = dev(ref), dev(org)
    # motion compensation, 16x16 luma PUs (the matrix-core kernel's shape)
    gx, gy = [a.reshape(-1) for a in np.meshgrid(np.arange(0, W, 16), np.arange(0, H, 16))]
    mc = np.zeros(gx.size, ops.MC_DESC)
    mc["ref0_off"] = mc["ref1_off"] = (gy + M) * (W + 2 * M) + gx + M
    mc["dst_off"] = gy * W + gx
    mc["ref0_stride"] = mc["ref1_stride"] = W + 2 * M
    mc["dst_stride"], mc["w"], mc["h"], mc["is_luma"], mc["bi"] = W, 16, 16, 1, 1
    mc["frac_x0"], mc["frac_y1"] = 4, 8
    dmc = ops.struct_to_device(mc)
    # fractional refinement, 16x16 blocks with the Hadamard cost
    fb = np.zeros(gx.size, ops.FRAC_BLK)
    mvx, mvy = rng.integers(-3, 4, gx.size), rng.integers(-3, 4, gx.size)
    fb["org_x"], fb["org_y"], fb["ref_x"], fb["ref_y"], fb["mv_x"], fb["mv_y"] = gx, gy, M + gx + mvx, M + gy + mvy, mvx, mvy
    dfb = ops.struct_to_device(fb)
    mv = ops.MvCost(17.0, 3, -2, 0, 0)
    # forward transform of 256 16x16 TUs, then 16384 4x4 TUs, over a 512 x 640 residual
    resi = rng.integers(-300, 300, (640, 512)).astype(np.int16)
    tr = [(y * 512 + x, 0, 512, 16, 16, 0, 0, 0, 0) for y in range(0, 128, 16) for x in range(0, 512, 16)]
    tr += [(y * 512 + x, 0, 512, 4, 4, 1, 1, 0, 0) for y in range(128, 640, 4) for x in range(0, 512, 4)]
    tr = np.array(tr, dtype=ops.TR_DESC)
    tr["coeff_off"] = np.concatenate([[0], np.cumsum(tr["w"].astype(np.int64) * tr["h"])[:-1]])
    dtr, dresi = ops.struct_to_device(tr), dev(resi)
    assert len(tr) >= 16384
    # residual chain of shape runs: 16x16 TUs, then 8x8 TUs
    tus = [(x, y, 16) for y in range(0, H // 2, 16) for x in range(0, W, 16)] + [(x, y, 8) for y in range(H // 2, H, 8) for x in range(0, W, 8)]
    rc = np.zeros(len(tus), ops.RC_DESC)
    for i, (x, y, s) in enumerate(tus):
        rc[i] = (y * W + x, y * W + x, y * W + x, 0, W, W, W, s, s, 0, 0, 0, 0, 32, (0, 0))
    rc["level_off"] = np.concatenate([[0], np.cumsum(rc["w"].astype(np.int64) * rc["h"])[:-1]])
    runs = [(16, 16, sum(t[2] == 16 for t in tus)), (8, 8, sum(t[2] == 8 for t in tus))]
    drc = ops.struct_to_device(rc)
    dpred = dev(np.ascontiguousarray(np.clip(org + rng.integers(-25, 26, org.shape), 0, mx).astype(np.int16)))

    def run_all():
        out = torch.zeros((H, W), dtype=torch.int16, device="cuda")
        ops.mc_batch(dref, dref, out, dmc, len(mc), bd, (0, mx))
        frac = ops.frac_refine(dorg, dref, dfb, len(fb), 16, 16, bd, mv, True, (0, mx))
        coeff = torch.zeros(int(tr["coeff_off"][-1]) + 16, dtype=torch.int32, device="cuda")
        ops.tr_fwd_batch(dresi, coeff, dtr, len(tr), bd)
        rec = dpred.clone()
        level = torch.zeros(int(rc["level_off"][-1]) + 64, dtype=torch.int32, device="cuda")
        asum = ops.resi_chain_runs_batch(dorg, dpred, rec, level, drc, len(rc), runs, bd, (0, mx))
        torch.cuda.synchronize()
        return [t.cpu().numpy() for t in (out, frac, coeff, rec, level, asum)]

    before = run_all()
    assert capi.lib().vvcgpu_shutdown() == 0, capi.lib().vvcgpu_last_error()
    after = run_all()
    for name, a, b in zip(("mc", "frac", "tr_fwd", "rec", "level", "abs_sum"), before, after):
        assert np.array_equal(a, b), name
    assert np.any(before[0] != 0) and np.any(before[2] != 0) and np.any(before[4] != 0)


def test_out_of_contract_descriptors_give_the_sentinel():
    """descriptors live in device memory, so the library cannot validate them on the host: the fused predict-and-distort kernels skip a descriptor whose
    shape does not fit their LDS tile and answer the documented sentinel ~0 (include/vvcgpu.h) instead of overrunning LDS; the valid neighbours of the
    bad descriptor in the same launch keep their exact results"""
    from vvcsoftware_vtm_amd import ops
    rng = np.random.default_rng(5)
    bd, mx, W, H = 10, 1023, 384, 320
    r0, org = cases.rand_plane(rng, H, W, bd, "smooth"), cases.rand_plane(rng, H, W, bd, "smooth")
    # vvcgpu_mc_dist_batch: w / h outside 1..128, bi outside 0..1
    good = (16 * W + 16, 16 * W + 16, 40 * W + 40, W, W, W, 16, 16, 4, 8, 0, 0, 1, 0, 0)
    rows = [good, (16 * W + 16, 16 * W + 16, 40 * W + 40, W, W, W, 200, 16, 0, 0, 0, 0, 1, 0, 0), good, (0, 0, 0, W, W, W, 16, 0, 0, 0, 0, 0, 1, 0, 0),
            (16 * W + 16, 16 * W + 16, 40 * W + 40, W, W, W, 16, 16, 0, 0, 0, 0, 1, 2, 0), good]
    d = np.array(rows, dtype=ops.MC_DESC)
    got = ops.mc_dist_batch(0, dev(r0), dev(r0), dev(org), ops.struct_to_device(d), len(d), bd, (0, mx)).cpu().numpy().view(np.uint64)
    assert got[1] == got[3] == got[4] == np.uint64(0xFFFFFFFFFFFFFFFF)
    assert got[0] == got[2] == got[5] and got[0] != np.uint64(0xFFFFFFFFFFFFFFFF)
    # vvcgpu_intra_satd_batch: w / h outside 1..64
    T, L = ops.intra_ref_lengths(16, 16)
    refs = rng.integers(0, mx + 1, 4 * (T + L + 1) + 600).astype(np.int16)
    sd = np.array([(0, 0, 24, 16, 16, 18, 0, 0, 0), (0, 0, 24, 128, 16, 18, 0, 0, 0), (0, 0, 24, 16, 16, 18, 0, 0, 0)], dtype=ops.INTRA_SATD_DESC)
    got = ops.intra_satd_batch(dev(refs), dev(org.reshape(-1)), ops.struct_to_device(sd), len(sd), clp=(0, mx)).cpu().numpy().view(np.uint64)
    assert got[1] == np.uint64(0xFFFFFFFFFFFFFFFF) and got[0] == got[2] != np.uint64(0xFFFFFFFFFFFFFFFF)


def test_warmup_builds_the_table_images_once():
    """vvcgpu_warmup: the per-device table images at a time the host chooses (idempotent); bit depths the kernels do not take are refused"""
    from vvcsoftware_vtm_amd import capi
    lib = capi.lib()
    for bd in (8, 10, 10):
        assert lib.vvcgpu_warmup(bd) == 0, lib.vvcgpu_last_error()
    assert lib.vvcgpu_warmup(12) == -3 and b"bit depth" in lib.vvcgpu_last_error()
