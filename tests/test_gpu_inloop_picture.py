"""GPU parity: the three-plane in-loop entry points (vvcgpu_sao_apply_picture, vvcgpu_sao_stats_picture, vvcgpu_alf_filter_picture,
vvcgpu_alf_stats_picture, vvcgpu_alf_classify_stats_picture) against the CPU oracle directly, plane by plane, at every CTU size the entry
points admit.  The shapes are chosen so that each kernel form is reached on purpose; the form is named in the test id."""
import numpy as np
import pytest
import torch

import cases
from oraclelib import oracle, p
from vvcsoftware_vtm_amd import capi

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A


def shapes(w, h):
    return [(h, w), (h // 2, w // 2), (h // 2, w // 2)]


def assert_plane(got, want, what):
    got = np.asarray(got)
    bad = got != want
    assert not bad.any(), "%s: %d of %d values differ, first at %s" % (what, int(bad.sum()), bad.size, tuple(int(i) for i in np.argwhere(bad)[0]))


class Views:
    """planes as views inside sentinel-filled device buffers: `col` columns and 2 rows of margin in front, `pad` columns behind"""

    def __init__(self, hw, col, pad, fill=None):
        self.bufs, self.views, self.col = [], [], col
        for i, (h, w) in enumerate(hw):
            b = torch.full((h + 4, col + w + pad), SENTINEL, dtype=torch.int16, device="cuda")
            v = b[2:2 + h, col:col + w]
            if fill is not None:
                v.copy_(torch.from_numpy(fill[i]))
            self.bufs.append(b)
            self.views.append(v)

    def check_margins(self, what):
        for i, (b, v) in enumerate(zip(self.bufs, self.views)):
            m = b.clone()
            m[2:2 + v.shape[0], self.col:self.col + v.shape[1]] = SENTINEL
            assert bool((m == SENTINEL).all()), "%s: plane %d written outside its view" % (what, i)


# ---- SAO apply -----------------------------------------------------------------------------------------------------------------
# forms of vvcgpu_sao_apply_picture: 'strip' = sao_apply_strip_kernel (width a multiple of 16, 16-byte aligned planes, strides multiples of 8);
# 'w8' = sao_apply_picture_kernel for a width that is not a multiple of 16; 'unaligned' = the same kernel for planes one column into a buffer
# whose stride is not a multiple of 8.  'strip' has whole 8-row bands in every plane (so a wave whose tile lies in one type takes the uniform walk
# everywhere); in 'strip_cut' the chroma height (60) cuts the band at the last row, and every chroma wave of a 32-column tile takes the general walk.
SAO_FORMS = {"strip": ((224, 144), 8, 8), "strip_cut": ((208, 120), 8, 8), "w8": ((200, 112), 8, 8), "unaligned": ((224, 128), 1, 3)}
SAO_MODES = ["type-1", "type0", "type1", "type2", "type3", "type4", "band4", "mixed", "edge_eo", "edge_bo"]


@pytest.mark.parametrize("mode", SAO_MODES)
@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("form", sorted(SAO_FORMS))
@pytest.mark.parametrize("ctu", [16, 32, 64, 128])
def test_sao_apply_picture(ctu, form, bd, mode):
    """every plane against orc_sao_apply with that plane's CTU (chroma CTU 8 / 16 / 32 / 64), partial availability, full and narrowed clipping;
    nothing outside the dst views changes"""
    from vvcsoftware_vtm_amd import ops
    (w, h), col, pad = SAO_FORMS[form]
    rng = np.random.default_rng([ctu, w, bd, SAO_MODES.index(mode)])
    mx = (1 << bd) - 1
    hw = shapes(w, h)
    src = [cases.rand_plane(rng, a, b, bd, "uniform" if i == 0 else "smooth") for i, (a, b) in enumerate(hw)]
    prms = cases.sao_picture_params(rng, w, h, ctu, mode)
    pdev = [ops.sao_params_to_device(q) for q in prms]
    for clp in ((0, mx), (64, 940) if bd == 10 else (16, 235)):
        s = Views(hw, col, pad, src)
        d = Views(hw, col, pad)
        ops.sao_apply_picture(s.views, d.views, ctu, bd, pdev, clp)
        for i, (a, b) in enumerate(hw):
            cs = ctu if i == 0 else ctu // 2
            want = src[i].copy()
            oracle().orc_sao_apply(p(src[i]), b, p(want), b, b, a, cs, cs, bd, p(prms[i]), clp[0], clp[1])
            assert_plane(d.views[i].cpu().numpy(), want, "plane %d clip %s" % (i, clp))
        d.check_margins("dst")
        s.check_margins("src")


def test_sao_apply_picture_bo_tiles_of_several_ctus_1080p():
    """band offset over a whole 1920x1080 picture at CTU 32 (every strip tile of every plane holds 4 to 16 CTUs) with the decoder binding's band
    layout, plus a picture at CTU 128 where each tile is one CTU"""
    from vvcsoftware_vtm_amd import ops
    for ctu in (32, 128):
        rng = np.random.default_rng(1080 + ctu)
        w, h, bd = 1920, 1080, 10
        hw = shapes(w, h)
        src = [cases.rand_plane(rng, a, b, bd, "smooth") for a, b in hw]
        prms = cases.sao_picture_params(rng, w, h, ctu, "band4")
        got = ops.sao_apply_picture([torch.from_numpy(x).cuda() for x in src], [torch.full(x.shape, -1, dtype=torch.int16, device="cuda") for x in src],
                                    ctu, bd, [ops.sao_params_to_device(q) for q in prms], (0, 1023))
        for i, (a, b) in enumerate(hw):
            cs = ctu if i == 0 else ctu // 2
            want = src[i].copy()
            oracle().orc_sao_apply(p(src[i]), b, p(want), b, b, a, cs, cs, bd, p(prms[i]), 0, 1023)
            assert_plane(got[i].cpu().numpy(), want, "ctu %d plane %d" % (ctu, i))


# ---- SAO statistics ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("skips", [(5, 4, 3, 2), (0, 0, 0, 0), (7, 1, 2, 5)], ids=["default", "none", "other"])
@pytest.mark.parametrize("use_avail", [False, True], ids=["geometry", "avail_map"])
@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("w,h", [(232, 136), (208, 120)])
@pytest.mark.parametrize("ctu", [32, 64, 128])
def test_sao_stats_picture(ctu, w, h, bd, use_avail, skips):
    """each plane against orc_sao_stats with that plane's CTU size and skip lines; partial CTUs at the right and bottom; an explicit
    availability map with cleared flags"""
    from vvcsoftware_vtm_amd import ops
    rng = np.random.default_rng([ctu, w, bd, int(use_avail), skips[0]])
    mx = (1 << bd) - 1
    hw = shapes(w, h)
    org = [cases.rand_plane(rng, a, b, bd, "smooth") for a, b in hw]
    rec = [np.clip(o.astype(np.int32) + rng.integers(-12, 13, o.shape), 0, mx).astype(np.int16) for o in org]
    rec[0] = cases.rand_plane(rng, h, w, bd, "flat")                # luma: many equal neighbours (EO sign 0), differences up to the full range
    nx, ny = cases.n_ctus(w, h, ctu)
    av = None
    if use_avail:
        av = np.zeros(nx * ny, np.uint8)
        for j in range(ny):
            for i in range(nx):
                av[j * nx + i] = (1 if i > 0 and rng.random() < 0.7 else 0) | (4 if j > 0 and rng.random() < 0.7 else 0) | \
                                 (16 if i > 0 and j > 0 and rng.random() < 0.7 else 0)
    got = ops.sao_stats_picture([torch.from_numpy(x).cuda() for x in org], [torch.from_numpy(x).cuda() for x in rec], ctu, bd,
                                None if av is None else torch.from_numpy(av).cuda(), skips[:2], skips[2:])
    for i, (a, b) in enumerate(hw):
        cs = ctu if i == 0 else ctu // 2
        sr, sb = skips[:2] if i == 0 else skips[2:]
        want = np.zeros((nx * ny, 5, 2, 32), np.int64)
        oracle().orc_sao_stats(p(org[i]), b, p(rec[i]), b, b, a, cs, cs, bd, p(av), sr, sb, p(want))
        assert_plane(got[i].cpu().numpy(), want, "plane %d" % i)


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("ctu", [32, 64, 128], ids=["scalar32_16", "packed64_scalar32", "packed128_64"])
def test_sao_stats_picture_one_category_full_ctu(ctu, bd):
    """the content of test_gpu_stats.py::test_sao_stats_one_category_full_ctu (|org - rec| = max everywhere, every sample of a CTU in one category or in
    the two extreme ones) in all three planes; one CTU and 2 x 2 CTUs with a partial last row and column, skip lines on and off, org and rec views with
    different strides.  The id names the body of the luma / chroma CTUs."""
    from vvcsoftware_vtm_amd import ops
    for (w, h) in ((ctu, ctu), (2 * ctu - 8, 2 * ctu - 12)):
        hw = shapes(w, h)
        nx, ny = cases.n_ctus(w, h, ctu)
        for kind in cases.SAO_ONE_CATEGORY_KINDS:
            pl = [cases.sao_one_category_planes(kind, b, a, bd) for a, b in hw]
            o = Views(hw, 8, 16, [q[0] for q in pl])
            r = Views(hw, 3, 7, [q[1] for q in pl])
            for skips in ((5, 4, 3, 2), (0, 0, 0, 0)):
                got = ops.sao_stats_picture(o.views, r.views, ctu, bd, None, skips[:2], skips[2:])
                for i, (a, b) in enumerate(hw):
                    cs = ctu if i == 0 else ctu // 2
                    sr, sb = skips[:2] if i == 0 else skips[2:]
                    want = np.zeros((nx * ny, 5, 2, 32), np.int64)
                    oracle().orc_sao_stats(p(pl[i][0]), b, p(pl[i][1]), b, b, a, cs, cs, bd, None, sr, sb, p(want))
                    assert_plane(got[i].cpu().numpy(), want, "%dx%d %s skips %s plane %d" % (w, h, kind, skips, i))


# ---- ALF filter ----------------------------------------------------------------------------------------------------------------
# variants: (content, coefficient amplitude, enables, narrowed clip).  'rand': a different random enable array per plane; 'null': NULL for all
# three; 'mix': luma and Cr random, Cb NULL
ALF_VARIANTS = {"rand": ("uniform", 60, "rand", False), "extreme": ("extreme", 200, "null", True), "mix": ("smooth", 60, "mix", True)}


def run_alf_filter_picture(w, h, ctu, ft, bd, variant, seed):
    from vvcsoftware_vtm_amd import ops
    kind, amp, en_mode, narrow = ALF_VARIANTS[variant]
    rng = np.random.default_rng(seed)
    mx = (1 << bd) - 1
    clp = ((64, 940) if bd == 10 else (16, 235)) if narrow else (0, mx)
    hw = shapes(w, h)
    src = [cases.rand_plane(rng, a, b, bd, kind) for a, b in hw]
    lc, cc = cases.alf_coeffs(rng, amp)
    if en_mode == "null":
        en = [None, None, None]
    else:
        en = [cases.ctu_enables(rng, w, h, ctu) for _ in range(3)]
        if en_mode == "mix":
            en[1] = None
    cls = np.zeros((h // 4, w // 4), np.uint16)
    oracle().orc_alf_classify(p(src[0]), w, w, h, bd, p(cls))
    s = Views(hw, 3, 5, src)                  # src: any alignment, garbage margins the filter must not read
    d = Views(hw, 4, 8)                       # dst: 8-byte aligned, stride a multiple of 4; disabled CTUs receive the unfiltered samples
    ops.alf_filter_picture(s.views, d.views, ctu, torch.from_numpy(cls.view(np.int16)).cuda(), ft, lc, cc,
                           [None if e is None else torch.from_numpy(e).cuda() for e in en], clp)
    for i, (a, b) in enumerate(hw):
        want = src[i].copy()
        if i == 0:
            oracle().orc_alf_filter_luma(p(src[0]), b, p(want), b, b, a, ctu, p(cls), ft, p(lc), p(en[0]), clp[0], clp[1])
        else:
            oracle().orc_alf_filter_chroma(p(src[i]), b, p(want), b, b, a, ctu // 2, p(cc), p(en[i]), clp[0], clp[1])
        assert_plane(d.views[i].cpu().numpy(), want, "plane %d" % i)
    d.check_margins("dst")


@pytest.mark.parametrize("variant", sorted(ALF_VARIANTS))
@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("ft", [0, 1])
@pytest.mark.parametrize("ctu", [16, 32, 64, 128])
def test_alf_filter_picture(ctu, ft, bd, variant):
    """luma and both chroma planes against orc_alf_filter_luma / _chroma (chroma CTU 8 .. 64), planes as views inside padded buffers"""
    run_alf_filter_picture(216, 136, ctu, ft, bd, variant, [ctu, ft, bd, sorted(ALF_VARIANTS).index(variant)])


def test_alf_filter_picture_1080p():
    run_alf_filter_picture(1920, 1080, 128, 1, 10, "mix", 1080)


# ---- ALF covariances -----------------------------------------------------------------------------------------------------------
def run_alf_stats_picture(w, h, ctu, bd, seed):
    """both luma sets and the Cb / Cr records of vvcgpu_alf_stats_picture and vvcgpu_alf_classify_stats_picture against orc_alf_stats"""
    from vvcsoftware_vtm_amd import ops
    rng = np.random.default_rng(seed)
    mx = (1 << bd) - 1
    hw = shapes(w, h)
    rec = [cases.rand_plane(rng, a, b, bd, "smooth" if i else "uniform") for i, (a, b) in enumerate(hw)]
    org = [np.clip(r.astype(np.int32) + rng.integers(-20, 21, r.shape), 0, mx).astype(np.int16) for r in rec]
    cls = np.zeros((h // 4, w // 4), np.uint16)
    oracle().orc_alf_classify(p(rec[0]), w, w, h, bd, p(cls))
    nx, ny = cases.n_ctus(w, h, ctu)
    want7 = np.zeros((nx * ny, 25, 183), np.int64)
    want5 = np.zeros((nx * ny, 25, 57), np.int64)
    oracle().orc_alf_stats(p(org[0]), w, p(rec[0]), w, w, h, ctu, p(cls), 1, p(want7))
    oracle().orc_alf_stats(p(org[0]), w, p(rec[0]), w, w, h, ctu, p(cls), 0, p(want5))
    wantc = []
    for i in (1, 2):
        a, b = hw[i]
        wc = np.zeros((nx * ny, 1, 57), np.int64)
        oracle().orc_alf_stats(p(org[i]), b, p(rec[i]), b, b, a, ctu // 2, None, 0, p(wc))
        wantc.append(wc)
    o = Views(hw, 4, 12, org)                 # org: 8-byte aligned, stride a multiple of 4; Cb and Cr strides equal
    r = Views(hw, 4, 12, rec)
    a7, a5, ac = ops.alf_stats_picture(o.views, r.views, ctu, torch.from_numpy(cls.view(np.int16)).cuda())
    gcls, f7, f5, fc = ops.alf_classify_stats_picture(o.views, r.views, ctu, bd)
    assert_plane(gcls.cpu().numpy().view(np.uint16), cls, "classes")
    for form, (g7, g5, gc) in (("alf_stats_picture", (a7, a5, ac)), ("alf_classify_stats_picture", (f7, f5, fc))):
        assert_plane(g7.cpu().numpy(), want7, form + " luma 7x7")
        assert_plane(g5.cpu().numpy(), want5, form + " luma 5x5")
        assert_plane(gc[0].cpu().numpy(), wantc[0], form + " Cb")
        assert_plane(gc[1].cpu().numpy(), wantc[1], form + " Cr")


# 64 / 128: the CTU form (fewer than 320 CTUs: the classifier's own launch in front); 256: the tile form with its separate chroma launch
@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("w,h", [(232, 136), (208, 120)])
@pytest.mark.parametrize("ctu", [64, 128, 256], ids=["ctu_form64", "ctu_form128", "tile_form256"])
def test_alf_stats_picture(ctu, w, h, bd):
    run_alf_stats_picture(w, h, ctu, bd, [ctu, w, bd])


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("w,h", [(0, 0), (136, 72)], ids=["one_ctu", "ragged"])
@pytest.mark.parametrize("ctu", [64, 128], ids=["ctu_form64", "ctu_form128"])
def test_alf_stats_picture_single_class_worst_limbs(ctu, w, h, bd):
    """the content of test_gpu_stats.py::test_alf_stats_single_class_worst_limbs through the CTU form (matrix-core Gram products on byte limbs, int32
    accumulators per class and CTU): every block of a CTU in one class at |org - rec| = max.  vvcgpu_alf_stats_picture with an all-zero class map (and an
    all-(24 | 3 << 8) one); vvcgpu_alf_classify_stats_picture with the classes it derives itself (constant / checkerboard planes: one class)."""
    from vvcsoftware_vtm_amd import ops
    from test_gpu_stats import alf_worst_kinds
    if w == 0:
        w = h = ctu
    hw = shapes(w, h)
    nx, ny = cases.n_ctus(w, h, ctu)
    for kind in alf_worst_kinds(bd):
        pl = [cases.alf_worst_planes(kind, b, a, bd) for a, b in hw]
        o = Views(hw, 4, 12, [q[0] for q in pl])
        r = Views(hw, 4, 12, [q[1] for q in pl])
        org, rec = pl[0]
        wantc = []
        for i in (1, 2):
            a, b = hw[i]
            wc = np.zeros((nx * ny, 1, 57), np.int64)
            oracle().orc_alf_stats(p(pl[i][0]), b, p(pl[i][1]), b, b, a, ctu // 2, None, 0, p(wc))
            wantc.append(wc)
        own = np.zeros((h // 4, w // 4), np.uint16)
        oracle().orc_alf_classify(p(rec), w, w, h, bd, p(own))
        assert len(np.unique(own & 0xFF)) == 1               # the classifier puts such a plane into ONE class (checkerboard: every transposition of it)
        maps = [("own", own), ("zero", np.zeros_like(own))] + ([("last", np.full_like(own, 24 | (3 << 8)))] if kind in (64, "checker") else [])
        for name, cls in maps:
            want7 = np.zeros((nx * ny, 25, 183), np.int64)
            want5 = np.zeros((nx * ny, 25, 57), np.int64)
            oracle().orc_alf_stats(p(org), w, p(rec), w, w, h, ctu, p(cls), 1, p(want7))
            oracle().orc_alf_stats(p(org), w, p(rec), w, w, h, ctu, p(cls), 0, p(want5))
            if name == "own":
                gcls, g7, g5, gc = ops.alf_classify_stats_picture(o.views, r.views, ctu, bd)
                assert_plane(gcls.cpu().numpy().view(np.uint16), cls, "classes")
            else:
                g7, g5, gc = ops.alf_stats_picture(o.views, r.views, ctu, torch.from_numpy(cls.view(np.int16)).cuda())
            what = "%s %s " % (kind, name)
            assert_plane(g7.cpu().numpy(), want7, what + "luma 7x7")
            assert_plane(g5.cpu().numpy(), want5, what + "luma 5x5")
            assert_plane(gc[0].cpu().numpy(), wantc[0], what + "Cb")
            assert_plane(gc[1].cpu().numpy(), wantc[1], what + "Cr")
            E = g7.cpu().numpy()[..., :169].reshape(-1, 13, 13)
            assert np.array_equal(E, E.transpose(0, 2, 1))
            assert int(g7.cpu().numpy()[..., -1].sum()) == int(((org.astype(np.int64) - rec) ** 2).sum())


def test_alf_stats_picture_1080p():
    run_alf_stats_picture(1920, 1080, 128, 10, 1081)


def test_alf_stats_picture_refuses_ctu_32():
    from vvcsoftware_vtm_amd import ops
    w, h = 64, 64
    pl = [torch.zeros(s, dtype=torch.int16, device="cuda") for s in shapes(w, h)]
    cls = torch.zeros((h // 4, w // 4), dtype=torch.int16, device="cuda")
    with pytest.raises(capi.VvcGpuError, match=r"failed \(-1\)"):
        ops.alf_stats_picture(pl, pl, 32, cls)
    with pytest.raises(capi.VvcGpuError, match=r"failed \(-1\)"):
        ops.alf_classify_stats_picture(pl, pl, 32, 10)
