"""CPU checks of the encoder picture analysis entries: the numpy restatement of tests/analysis_cases.py against the compiled reference's outputs
(tests/golden/analysis.npz), the library's host finishers against both, and the argument checks of every new entry (no device is touched).  The layouts
of the two structs: tests/test_abi.py."""
import ctypes as C
import os

import numpy as np
import pytest

import analysis_cases as ac
from vvcsoftware_vtm_amd import abi, capi

G = os.path.join(os.path.dirname(__file__), "golden")
PLANES = [(w, h, k) for (w, h) in ac.GOLDEN_PLANES for k in ac.KINDS] + [(1920, 1080, "big"), (960, 540, "big")]


def _lib():
    if not os.path.exists(capi.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return capi.lib()


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(G, "analysis.npz"))


def plane(gold, bd, w, h, kind):
    if kind == "big":
        return ac.big_plane(gold["bd%d_64x64_noise_org" % bd], h, w, bd)
    return gold["bd%d_%dx%d_%s_org" % (bd, w, h, kind)]


def test_fixture_covers_the_block_sizes_and_contents(gold):
    got = {ac.wpsnr_block_size(w, h, cs) for (w, h, _) in PLANES for cs in (0, 1)}
    assert got >= {64, 32, 16, 8, 4, 0}
    assert [ac.wpsnr_block_size(*s) for s in [(3840, 2160, 0), (1920, 1080, 1), (7680, 4320, 0), (3840, 2160, 1), (1920, 1080, 0), (960, 540, 1),
                                              (416, 240, 0), (208, 120, 1), (208, 120, 0), (104, 60, 1), (64, 64, 0), (32, 32, 1), (32, 32, 0)]] \
        == [128, 64, 128, 64, 64, 32, 16, 8, 8, 4, 4, 0, 0]
    for bd in (8, 10):
        lim = float(1 << (bd - 4))
        assert gold["bd%d_416x240_flat_plane_ener" % bd] == lim and (gold["bd%d_416x240_flat_qpa64_ener" % bd] == lim).all()      # below the lower limit
        assert gold["bd%d_416x240_noise_plane_ener" % bd] > lim
        b = gold["bd%d_416x240_border_org" % bd]
        assert not b[0].any() and not b[:, -1].any() and b[120, 200] > 0


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("w,h,kind", PLANES)
def test_restatement_equals_reference(gold, bd, w, h, kind):
    k = "bd%d_%dx%d_%s_" % (bd, w, h, kind)
    org = plane(gold, bd, w, h, kind)
    rec, ref = ac.rec_of(org, bd), ac.ref_of(org, bd)
    assert ac.sse(org, rec) == int(gold[k + "sse"])
    whole = int(ac.highpass_abs(org).sum())
    assert float(ac.energy(whole, (w - 2) * (h - 2), bd)) == float(gold[k + "plane_ener"])
    for t in ac.CTU_SIZES:
        s = ac.tile_stats(org, rec, t)
        assert np.array_equal(ac.energy(s[..., 0], ac.tile_act_count(h, w, t), bd), gold[k + "qpa%d_ener" % t]), t
        assert np.array_equal(ac.ctu_dc(s, h, w, t), gold[k + "qpa%d_dc" % t]), t
        # per tile -> whole plane: the activity of applyQPAdaptationChroma, the luma mean, the plain SSE
        assert int(s[..., 0].sum()) == whole and int(s[..., 1].sum()) == int(org.astype(np.int64).sum()) and int(s[..., 2].sum()) == int(gold[k + "sse"])
    assert np.array_equal(ac.histogram(org, bd), gold[k + "hist"].astype(np.uint32))
    assert [ac.wp_sad(org, ref, bd, c) for c in ac.wp_cands(bd)] == [int(v) for v in gold[k + "wp_sad"]]
    for cs in (0, 1):
        assert ac.wpsnr_plane(org, rec, cs, bd) == int(gold[k + "wpsnr_cs%d" % cs]), cs


@pytest.mark.parametrize("bd", [8, 10])
def test_restatement_of_acdc_and_intra_cost_equals_reference(gold, bd):
    for i, kind in enumerate(ac.KINDS):
        pls = [plane(gold, bd, 416, 240, kind), plane(gold, bd, 208, 120, kind), plane(gold, bd, 208, 120, ac.KINDS[(i + 1) % 4])]
        want = gold["bd%d_acdc_%s" % (bd, kind)]
        for c, pl in enumerate(pls):
            for hp in (0, 1):
                assert ac.wp_acdc(ac.histogram(pl, bd), pl.size, 0) == ac.wp_acdc_direct(pl, 0) == (int(want[hp, 2 * c]), int(want[hp, 2 * c + 1]))
    for (w, h) in ac.INTRA_SIZES:
        for kind in ("noise", "gradient"):
            org = plane(gold, bd, 416, 240, kind)[:h, :w]
            for ctu in (128, 64):
                assert np.array_equal(ac.intra_cost(org, ctu, bd), gold["bd%d_intra_%dx%d_%s_ctu%d" % (bd, w, h, kind, ctu)]), (w, h, kind, ctu)


def _finish(lib, stats, w, h, cs, bd):
    t = np.ascontiguousarray(stats.reshape(-1, 3).astype(np.uint64))
    assert t.view(abi.TILE_STATS).shape == (t.shape[0], 1)
    ssd = C.c_uint64()
    rc = lib.vvcgpu_wpsnr_finish_host(t.ctypes.data_as(C.c_void_p), w, h, cs, bd, C.byref(ssd))
    assert rc == 0, lib.vvcgpu_last_error()
    return ssd.value


def _block_size(lib, w, h, cs):
    b = C.c_int(-1)
    assert lib.vvcgpu_wpsnr_block_size_host(w, h, cs, C.byref(b)) == 0
    return b.value


def test_block_size_helper():
    lib = _lib()
    for (w, h) in [(3840, 2160), (7680, 4320), (1920, 1080), (1280, 720), (960, 540), (416, 240), (208, 120), (104, 60), (64, 64), (40, 24), (32, 32), (8, 8)]:
        for cs in (0, 1):
            assert _block_size(lib, w, h, cs) == ac.wpsnr_block_size(w, h, cs), (w, h, cs)
    assert [_block_size(lib, *s) for s in [(3840, 2160, 0), (1920, 1080, 1), (1920, 1080, 0), (960, 540, 1), (416, 240, 0), (208, 120, 1), (208, 120, 0),
                                           (104, 60, 1), (64, 64, 0), (32, 32, 1), (32, 32, 0)]] == [128, 64, 64, 32, 16, 8, 8, 4, 4, 0, 0]


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("w,h,kind", PLANES)
def test_wpsnr_finisher_equals_restatement_and_reference(gold, bd, w, h, kind):
    """the C finisher == the restatement evaluated on this machine (math.pow) == the reference's final"""
    lib = _lib()
    org = plane(gold, bd, w, h, kind)
    rec = ac.rec_of(org, bd)
    for cs in (0, 1):
        b = ac.wpsnr_block_size(w, h, cs)
        want = int(gold["bd%d_%dx%d_%s_wpsnr_cs%d" % (bd, w, h, kind, cs)])
        if b == 0:                                                     # the reference takes the plain SSE; the finisher refuses the plane
            assert want == ac.sse(org, rec)
            ssd = C.c_uint64()
            assert lib.vvcgpu_wpsnr_finish_host(C.c_void_p(4096), w, h, cs, bd, C.byref(ssd)) == -1 and b"wpsnr_finish_host" in lib.vvcgpu_last_error()
            continue
        s = ac.tile_stats(org, rec, b)
        assert _finish(lib, s, w, h, cs, bd) == ac.wpsnr_finish(s, w, h, cs, bd) == want, (cs, b)


def test_wpsnr_finisher_large_pictures_and_zero_error():
    """4K (the 0.5 scaling of :2785-2788) and a zero error (wmse <= 0 -> 0): C finisher == restatement"""
    lib = _lib()
    rng = np.random.default_rng(3)
    for (w, h, cs) in [(3840, 2160, 0), (1920, 1080, 1), (1280, 720, 0)]:
        for bd in (8, 10):
            b = ac.wpsnr_block_size(w, h, cs)
            n = (-(-h // b)) * (-(-w // b))
            s = np.stack([rng.integers(0, 12 * 1023 * b * b, n), rng.integers(0, 1023 * b * b, n), rng.integers(0, 1023 * 1023 * b * b, n)], axis=-1).astype(np.uint64)
            assert _finish(lib, s, w, h, cs, bd) == ac.wpsnr_finish(s, w, h, cs, bd) > 0
            s[:, 2] = 0
            assert _finish(lib, s, w, h, cs, bd) == 0


@pytest.mark.parametrize("bd", [8, 10])
def test_acdc_helper_equals_restatement_and_reference(gold, bd):
    lib = _lib()
    for i, kind in enumerate(ac.KINDS):
        pls = [plane(gold, bd, 416, 240, kind), plane(gold, bd, 208, 120, kind), plane(gold, bd, 208, 120, ac.KINDS[(i + 1) % 4])]
        want = gold["bd%d_acdc_%s" % (bd, kind)]
        for c, pl in enumerate(pls):
            hist = np.ascontiguousarray(ac.histogram(pl, bd))
            for shift in (0, 4):
                dc, acv = C.c_int64(), C.c_int64()
                assert lib.vvcgpu_wp_acdc_host(hist.ctypes.data_as(C.c_void_p), bd, pl.size, shift, C.byref(dc), C.byref(acv)) == 0
                assert (dc.value, acv.value) == ac.wp_acdc(hist, pl.size, shift) == ac.wp_acdc_direct(pl, shift)
                if shift == 0:
                    assert (dc.value, acv.value) == (int(want[0, 2 * c]), int(want[0, 2 * c + 1]))
    dc, acv = C.c_int64(), C.c_int64()
    hist = np.zeros(1 << bd, np.uint32)
    hist[5] = 7
    assert lib.vvcgpu_wp_acdc_host(hist.ctypes.data_as(C.c_void_p), bd, 8, 0, C.byref(dc), C.byref(acv)) == -1 and b"wp_acdc_host" in lib.vvcgpu_last_error()


def test_analysis_argument_checks_need_no_device():
    lib = _lib()
    P = C.c_void_p(4096)                     # never dereferenced: every check below fails before device work
    good, nul = abi.Planes(), abi.Planes()
    for c in range(3):
        good.p[c] = 4096
        good.stride[c] = 416 if c == 0 else 208
    G_, N_ = C.byref(good), C.byref(nul)
    short = abi.Planes()
    for c in range(3):
        short.p[c] = 4096
        short.stride[c] = 100
    S_ = C.byref(short)
    err = lambda: lib.vvcgpu_last_error()

    ts = lambda *a: lib.vvcgpu_tile_stats_picture(*a)
    for a in ([None, None, 416, 240, 64, 3, P, P, P, None], [G_, None, 416, 240, 64, 3, None, P, P, None], [G_, None, 416, 240, 64, 3, P, None, P, None],
              [G_, None, 416, 240, 64, 3, P, P, None, None], [N_, None, 416, 240, 64, 3, P, P, P, None], [G_, N_, 416, 240, 64, 3, P, P, P, None],
              [S_, None, 416, 240, 64, 3, P, P, P, None], [G_, None, 0, 240, 64, 3, P, P, P, None], [G_, None, 416, -1, 64, 3, P, P, P, None],
              [G_, None, 415, 240, 64, 3, P, P, P, None], [G_, None, 416, 240, 64, 2, P, P, P, None], [G_, None, 416, 240, 0, 3, P, P, P, None],
              [G_, None, 416, 240, 4, 3, P, P, P, None], [G_, None, 416, 240, 6, 1, P, None, None, None], [G_, None, 416, 240, 256, 1, P, None, None, None]):
        assert ts(*a) == -1 and b"tile_stats_picture" in err(), a

    se = lambda *a: lib.vvcgpu_picture_sse(*a)
    for a in ([None, G_, 416, 240, 3, P, None], [G_, None, 416, 240, 3, P, None], [G_, G_, 416, 240, 3, None, None], [G_, N_, 416, 240, 3, P, None],
              [G_, S_, 416, 240, 1, P, None], [G_, G_, 416, 240, 0, P, None], [G_, G_, 416, 0, 3, P, None], [G_, G_, 416, 241, 3, P, None]):
        assert se(*a) == -1 and b"picture_sse" in err(), a

    hi = lambda *a: lib.vvcgpu_picture_histogram(*a)
    for a in ([None, 416, 240, 3, 10, P, None], [G_, 416, 240, 3, 10, None, None], [N_, 416, 240, 1, 10, P, None], [S_, 416, 240, 3, 10, P, None],
              [G_, 416, 240, 2, 10, P, None], [G_, 0, 240, 3, 10, P, None]):
        assert hi(*a) == -1 and b"picture_histogram" in err(), a
    for bd in (7, 11, 12):
        assert hi(G_, 416, 240, 3, bd, P, None) == -3 and b"picture_histogram" in err() and b"bit depth" in err()

    cands = np.array([(6, 64, 0, 0)] * 17, dtype=abi.WP_SAD_CAND)
    cp = cands.ctypes.data_as(C.c_void_p)
    ws = lambda *a: lib.vvcgpu_wp_sad_batch(*a)
    assert ws(None, 0, None, 0, 0, 0, 10, None, 0, None, None) == 0                                      # n_cand == 0: a no-op
    for a in ([None, 416, P, 416, 416, 240, 10, cp, 4, P, None], [P, 416, None, 416, 416, 240, 10, cp, 4, P, None], [P, 416, P, 416, 416, 240, 10, None, 4, P, None],
              [P, 416, P, 416, 416, 240, 10, cp, 4, None, None], [P, 416, P, 416, 416, 240, 10, cp, 17, P, None], [P, 416, P, 416, 416, 240, 10, cp, -1, P, None],
              [P, 400, P, 416, 416, 240, 10, cp, 4, P, None], [P, 416, P, 415, 416, 240, 10, cp, 4, P, None], [P, 416, P, 416, 0, 240, 10, cp, 4, P, None]):
        assert ws(*a) == -1 and b"wp_sad_batch" in err(), a
    for bad in [(8, 64, 0, 0), (-1, 64, 0, 0), (6, 1025, 0, 0), (6, -1025, 0, 0), (6, 64, 32768, 0), (6, 64, -32769, 0), (6, 64, 0, 4)]:
        c1 = np.array([(6, 64, 0, 0), bad], dtype=abi.WP_SAD_CAND)
        assert ws(P, 416, P, 416, 416, 240, 10, c1.ctypes.data_as(C.c_void_p), 2, P, None) == -1 and b"candidate 1" in err(), bad
    for bd in (7, 11):
        assert ws(P, 416, P, 416, 416, 240, bd, cp, 4, P, None) == -3 and b"wp_sad_batch" in err() and b"bit depth" in err()

    ic = lambda *a: lib.vvcgpu_intra_cost_ctus(*a)
    for a in ([None, 416, 416, 240, 128, 10, P, None], [P, 416, 416, 240, 128, 10, None, None], [P, 415, 416, 240, 128, 10, P, None],
              [P, 416, 0, 240, 128, 10, P, None], [P, 416, 416, 240, 100, 10, P, None], [P, 416, 416, 240, 8, 10, P, None], [P, 416, 416, 240, 256, 10, P, None]):
        assert ic(*a) == -1 and b"intra_cost_ctus" in err(), a
    for bd in (7, 11):
        assert ic(P, 416, 416, 240, 128, bd, P, None) == -3 and b"intra_cost_ctus" in err() and b"bit depth" in err()

    b = C.c_int()
    ssd = C.c_uint64()
    assert lib.vvcgpu_wpsnr_block_size_host(416, 240, 0, None) == -1 and b"wpsnr_block_size_host" in err()
    assert lib.vvcgpu_wpsnr_block_size_host(0, 240, 0, C.byref(b)) == -1 and lib.vvcgpu_wpsnr_block_size_host(416, 240, 2, C.byref(b)) == -1
    assert lib.vvcgpu_wpsnr_finish_host(None, 416, 240, 0, 10, C.byref(ssd)) == -1 and b"wpsnr_finish_host" in err()
    assert lib.vvcgpu_wpsnr_finish_host(P, 416, 240, 0, 10, None) == -1
    assert lib.vvcgpu_wpsnr_finish_host(P, 416, 240, 0, 12, C.byref(ssd)) == -3 and b"bit depth" in err()
    assert lib.vvcgpu_wp_acdc_host(None, 10, 100, 0, C.byref(C.c_int64()), C.byref(C.c_int64())) == -1 and b"wp_acdc_host" in err()
    assert lib.vvcgpu_wp_acdc_host(P, 11, 100, 0, C.byref(C.c_int64()), C.byref(C.c_int64())) == -3
    assert lib.vvcgpu_wp_acdc_host(P, 10, 0, 0, C.byref(C.c_int64()), C.byref(C.c_int64())) == -1
