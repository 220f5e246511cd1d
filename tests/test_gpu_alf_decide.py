"""GPU parity of vvcgpu_alf_frame_stats and vvcgpu_alf_ctu_dist, through the C ABI: against the compiled reference's results of
tests/golden/alf_decide.npz where the fixture covers the case, against the restatement of tests/alf_decide_cases.py (which the fixture pins to the
reference, tests/test_alf_decide_cpu.py) everywhere else.  Frame sums are compared as int64, distortions as the 64-bit patterns of their doubles."""
import functools
import os

import numpy as np
import pytest
import torch

import alf_decide_cases as adc
from oraclelib import oracle, p
from vvcsoftware_vtm_amd import ops

pytestmark = pytest.mark.gpu

CASES = adc.load_golden()
POISON = 0x5A5A5A5A5A5A5A5A
SLICE = 8                      # CTUs per workgroup slice of alf_frame_stats_kernel (FS_SLICE in csrc/alfdecide.hip): 7, 8 and 9 CTUs are below, at and above it
FRAME_N_CTU = [1, 2, 6, SLICE - 1, SLICE, SLICE + 1, 37, 510]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def assert_bits(got, want, what):
    got, want = adc.bits(got.cpu().numpy() if torch.is_tensor(got) else got), adc.bits(want)
    bad = (got != want).any(1)
    assert not bad.any(), "%s: %d of %d CTUs differ, first %d: got %r, want %r" % (
        what, int(bad.sum()), bad.size, int(np.nonzero(bad)[0][0]), got[bad][0].view(np.float64).tolist(), want[bad][0].view(np.float64).tolist())


def assert_frame(got, want, what):
    got = got.cpu().numpy()
    bad = got != want
    assert not bad.any(), "%s: %d of %d sums differ, first at %s" % (what, int(bad.sum()), bad.size, tuple(int(i) for i in np.argwhere(bad)[0]))


@functools.lru_cache(maxsize=None)
def noise510(n_cls, filter_type):
    """510 CTUs (a 4K picture of 128x128 CTUs) of the noise set, on the host and on the device; the smaller counts are its leading CTUs"""
    rec = adc.records(adc.NOISE, 5, 510, n_cls, filter_type)
    rec_d = dev(rec)
    rec.setflags(write=False)
    return rec, rec_d


# ---- frame sums ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_cls,filter_type", [(25, 1), (25, 0), (1, 0)], ids=["25x183", "25x57", "1x57"])
def test_frame_stats(n_cls, filter_type):
    """every CTU count x {no mask, all off, mixed}; the output starts poisoned, so a sum that is not written or not cleared shows"""
    rec, rec_d = noise510(n_cls, filter_type)
    for n in FRAME_N_CTU:
        for mode in (None, "off", "mixed"):
            en = None if mode is None else adc.enable_mask(n, n, mode)
            out = torch.full(rec.shape[1:], POISON, dtype=torch.int64, device="cuda")
            got = ops.alf_frame_stats(rec_d[:n], None if en is None else dev(en), out=out)
            assert_frame(got, adc.frame_stats(rec[:n], en), "%d CTUs, mask %s" % (n, mode))


@pytest.mark.parametrize("c", CASES, ids=[c["id"] for c in CASES])
def test_frame_stats_golden(c):
    got = ops.alf_frame_stats(dev(adc.case_records(c)), dev(c["enable"]))
    assert_frame(got, c["frame"], "getFrameStat")


def test_frame_stats_chroma_accumulates_cb_then_cr():
    """the chroma frame record of getFrameStats (:1298-1299): Cb overwrites, Cr adds"""
    cb, cr = adc.records(adc.NOISE, 31, 37, 1, 0), adc.records(adc.NOISE, 32, 37, 1, 0)
    en_cb, en_cr = adc.enable_mask(31, 37, "mixed"), adc.enable_mask(32, 37, "mixed")
    out = torch.full((1, 57), POISON, dtype=torch.int64, device="cuda")
    ops.alf_frame_stats(dev(cb), dev(en_cb), out=out)
    ops.alf_frame_stats(dev(cr), dev(en_cr), out=out, accumulate=True)
    assert_frame(out, adc.frame_stats(cb, en_cb) + adc.frame_stats(cr, en_cr), "Cb + Cr")
    ops.alf_frame_stats(dev(cr), None, out=out, accumulate=True)
    assert_frame(out, adc.frame_stats(cb, en_cb) + adc.frame_stats(cr, en_cr) + adc.frame_stats(cr), "Cb + Cr + Cr")


def test_frame_stats_back_to_back_on_one_stream():
    """two calls with different masks, no synchronisation between them, the second into the first's output as well: nothing of the first survives"""
    rec, rec_d = noise510(25, 0)
    n = 37
    m1, m2 = adc.enable_mask(1, n, "mixed"), adc.enable_mask(2, n, "mixed")
    assert not np.array_equal(m1, m2)
    m1_d, m2_d = dev(m1), dev(m2)
    out1 = ops.alf_frame_stats(rec_d[:n], m1_d)
    out2 = ops.alf_frame_stats(rec_d[:n], m2_d)
    reused = ops.alf_frame_stats(rec_d[:n], m1_d)
    ops.alf_frame_stats(rec_d[:n], m2_d, out=reused)
    assert_frame(out1, adc.frame_stats(rec[:n], m1), "first call")
    assert_frame(out2, adc.frame_stats(rec[:n], m2), "second call")
    assert_frame(reused, adc.frame_stats(rec[:n], m2), "second call into the first's output")


# ---- per-CTU distortions -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", CASES, ids=[c["id"] for c in CASES])
def test_ctu_dist_golden(c):
    """the reference's getUnfilteredDistortion / getFilteredDistortion, bit for bit -- the large set among them, on which a reordered sum fails"""
    got = ops.alf_ctu_dist(dev(adc.case_records(c)), c["coeff"], c["idx"] if c["n_cls"] > 1 else None, c["coeff_bits"])
    assert_bits(got, c["dist"], "against the reference")


# (n_ctu, n_filters, coeff_bits)
DIST_RUNS = [(1, 1, 10), (6, 3, 10), (37, 25, 10), (37, 3, 12), (510, 3, 10), (510, 25, 11)]


@pytest.mark.parametrize("n_cls", [25, 1])
@pytest.mark.parametrize("filter_type", [0, 1], ids=["5x5", "7x7"])
@pytest.mark.parametrize("kind", [adc.REAL, adc.NOISE, adc.LARGE], ids=["real", "noise", "large"])
def test_ctu_dist(kind, filter_type, n_cls):
    N = adc.N_OF[filter_type]
    for n, n_filters, coeff_bits in DIST_RUNS:
        rec = adc.records(kind, 40 + n_filters, n, n_cls, filter_type, n_filters, coeff_bits)
        coeff = adc.coeff_set(40 + n_filters, n_filters, N)
        if n_filters == 3:
            coeff[2] = 0
        idx = adc.filter_indices(40 + n_filters, n_cls, n_filters) if n_cls > 1 else None
        got = ops.alf_ctu_dist(dev(rec), coeff, idx, coeff_bits)
        assert_bits(got, adc.ctu_dist(rec, coeff, idx, coeff_bits), "%d CTUs, %d filters, %d bits" % (n, n_filters, coeff_bits))


def test_ctu_dist_unaligned_records():
    """a record set that starts 8 bytes off a 16-byte boundary (every second CTU of an odd-sized record does anyway): both phases of the LDS copy"""
    rec = adc.records(adc.LARGE, 9, 6, 25, 1, 3, 10)
    coeff, idx = adc.coeff_set(9, 3, 13), adc.filter_indices(9, 25, 3)
    buf = torch.zeros(rec.size + 1, dtype=torch.int64, device="cuda")
    want = adc.ctu_dist(rec, coeff, idx)
    for off in (0, 1):
        view = buf[off:off + rec.size].view(rec.shape)
        view.copy_(dev(rec))
        assert view.data_ptr() % 16 == 8 * off
        assert_bits(ops.alf_ctu_dist(view, coeff, idx), want, "offset %d" % off)


# ---- behind the statistics launch ----------------------------------------------------------------------------------------------------------------
def test_composed_with_classify_stats_picture():
    """the 136x72 picture c0 of alf.npz: vvcgpu_alf_classify_stats_picture's device outputs go straight into both entries; compared with the
    restatement applied to the oracle's records (orc_alf_stats)"""
    g = np.load(os.path.join(adc.HERE, "golden", "alf.npz"))
    w, h, ctu, bd = (int(v) for v in g["c0_meta"])
    rng = np.random.default_rng(136)
    rec = [g["c0_Y"], g["c0_Cb"], g["c0_Cr"]]
    org = [g["c0_org"]] + [np.clip(r.astype(np.int32) + rng.integers(-20, 21, r.shape), 0, (1 << bd) - 1).astype(np.int16) for r in rec[1:]]
    cls = np.ascontiguousarray(g["c0_cls_all"])
    n = ((w + ctu - 1) // ctu) * ((h + ctu - 1) // ctu)
    want = {}
    for ft, key in ((1, "y7"), (0, "y5")):
        want[key] = np.zeros((n, 25, adc.n_vals(adc.N_OF[ft])), np.int64)
        oracle().orc_alf_stats(p(org[0]), w, p(rec[0]), w, w, h, ctu, p(cls), ft, p(want[key]))
    for i, key in ((1, "cb"), (2, "cr")):
        want[key] = np.zeros((n, 1, 57), np.int64)
        oracle().orc_alf_stats(p(org[i]), w // 2, p(rec[i]), w // 2, w // 2, h // 2, ctu // 2, None, 0, p(want[key]))
    assert np.array_equal(want["y7"], g["c0_stats_f1"])                      # the oracle's records are the reference's

    _, a7, a5, ac = ops.alf_classify_stats_picture([dev(a) for a in org], [dev(a) for a in rec], ctu, bd)
    en = {k: g["c0_en" + k] for k in ("Y", "Cb", "Cr")}
    lc, cc = g["c0_lc"].astype(np.int32), g["c0_cc"].astype(np.int32).reshape(1, 7)
    idx = np.arange(25, dtype=np.int16)
    assert_frame(ops.alf_frame_stats(a7, dev(en["Y"])), adc.frame_stats(want["y7"], en["Y"]), "luma 7x7 frame")
    assert_frame(ops.alf_frame_stats(a5, dev(en["Y"])), adc.frame_stats(want["y5"], en["Y"]), "luma 5x5 frame")
    chroma = ops.alf_frame_stats(ac[0], dev(en["Cb"]))
    ops.alf_frame_stats(ac[1], dev(en["Cr"]), out=chroma, accumulate=True)
    assert_frame(chroma, adc.frame_stats(want["cb"], en["Cb"]) + adc.frame_stats(want["cr"], en["Cr"]), "chroma frame")
    assert_bits(ops.alf_ctu_dist(a7, lc, idx), adc.ctu_dist(want["y7"], lc, idx), "luma 7x7 distortions")
    assert_bits(ops.alf_ctu_dist(a5, lc[:, :7], idx), adc.ctu_dist(want["y5"], lc[:, :7], idx), "luma 5x5 distortions")
    for k, a in (("cb", ac[0]), ("cr", ac[1])):
        assert_bits(ops.alf_ctu_dist(a, cc), adc.ctu_dist(want[k], cc, None), k + " distortions")
