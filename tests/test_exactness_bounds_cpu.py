"""CPU: the worst-case inputs of tests/cases.py really sit on the bounds the device kernels' exactness arguments name (csrc/mfma_tr.h, csrc/resichain.hip,
csrc/saostats.hip, csrc/alfstats.hip).  The device tests at those bounds (test_tr_fwd_inv_at_the_exactness_bound, test_resi_chain_at_the_exactness_bound,
test_sao_stats_one_category_full_ctu, ...) use the same builders and rely on what is asserted here."""
import numpy as np

import cases
from oraclelib import oracle, p


def stage1(row):
    """|X Th^T| of a forward item in int64, and the first stage's rounded result as the reference computes it"""
    w, h, th, tv, k, l, negate, amp, bd = (int(v) for v in row)
    x = cases.tr_aligned_block(w, h, th, tv, k, l, amp, bool(negate)).astype(np.int64)
    s = x @ cases.tr_matrix(th, w)[:min(w, 32)].T
    s1 = int(np.log2(w)) + bd + 6 - 15 + 2
    return np.abs(s), (s + (1 << (s1 - 1))) >> s1


def test_forward_items_reach_the_f32_and_the_16_bit_bounds():
    rows = cases.tr_worst_rows()
    top10 = max(int(stage1(r)[0].max()) for r in rows if r[8] == 10 and r[0] == 64)
    assert top10 == 16760832 == (1 << 24) - 16384          # 1023 x the DCT-II 64 row-sum of |c|: the f32 accumulator's margin
    wide8 = max(int(np.abs(stage1(r)[1]).max()) for r in rows if r[8] == 8 and r[7] == 1023 and r[0] == 64)
    assert wide8 == 130944 > 65535                          # bit depth 8 at +-1023: the first stage's result is no 16-bit operand
    # ... and the second stage's recombination (hi << 8) + lo of a 64-row column of such values stays inside int32
    assert 130944 * 16384 == 2145386496 < (1 << 31)


def test_forward_items_reach_the_limb_edge():
    """a coefficient (and a first-stage result) of +-32736: limbs hi = +-128, lo = -+32, the edge of rc_limbs"""
    O = oracle()
    hit = set()
    for row in cases.tr_worst_rows():
        w, h, th, tv, k, l, negate, amp, bd = (int(v) for v in row)
        if bd != 10 or (w, h) != (64, 64):
            continue
        r = np.ascontiguousarray(cases.tr_aligned_block(w, h, th, tv, k, l, amp, bool(negate)))
        c = np.zeros(w * h, np.int32)
        O.orc_tr_fwd(p(r), w, p(c), w, h, th, tv, bd)
        hit |= {int(c.max()), int(c.min())} & {32736, -32736}
        if (k, l) == (0, 0):
            assert int(np.abs(stage1(row)[1]).max()) == 32736
    assert hit == {32736, -32736}


def test_inverse_items_are_full_scale():
    rows = cases.tr_worst_inv_rows()
    assert {int(r[6]) for r in rows} == {32767, -32768}
    c = cases.tr_aligned_coeffs(64, 64, 0, 0, 63, 63, 32767)
    assert np.all(np.abs(c[:32, :32]) == 32767) and not c[32:].any() and not c[:, 32:].any()
    for val, lim in ((32767, 32767), (-32768, -32768)):     # both clips of the inverse transform bind at the aligned sample
        c = np.ascontiguousarray(cases.tr_aligned_coeffs(64, 64, 0, 0, 63, 63, val))
        want = np.zeros((64, 64), np.int16)
        oracle().orc_tr_inv(p(c), p(want), 64, 64, 64, 0, 0, 10)
        assert int(want[63, 63]) == lim


def test_low_qp_chain_list_reaches_the_level_clip():
    from test_gpu_resichain import oracle_chain
    org, pred, tus, W = cases.chain_bound_case(10)
    lv, asum, rec, coffs = oracle_chain(org, pred, tus, 10, W)
    top, low, wider = set(), set(), 0
    for i, t in enumerate(tus):
        l = lv[coffs[i]:coffs[i] + t[2] * t[3]]
        if int(l.max()) == 32767:
            top.add((t[2], t[3]))
        if int(l.min()) == -32768:                           # Quant::quant clips to -32768 .. 32767
            low.add((t[2], t[3]))
        wider += int(np.abs(l).max()) >= 32767 and int(asum[i]) > int(np.abs(l.astype(np.int64)).sum()) + 1    # (+ 1: sign hiding moves one level by one)
    assert {(64, 64), (32, 32)} <= top and {(64, 64), (32, 32)} <= low
    assert wider > 0                                         # abs_sum adds the magnitudes BEFORE the clip
    i = next(i for i, t in enumerate(tus) if t[2:4] == (64, 64) and t[6] == 0 and int(lv[coffs[i]]) == 32767)
    assert int(asum[i]) == 104753
    assert {t[6] for t in tus} == {0, 12, 16, 24, 34} and {t[7] for t in tus} == {0, 1} and {t[8] for t in tus} == {0, 1}
    assert len({(t[2], t[3]) for t in tus}) == 29


def test_sao_planes_put_a_full_ctu_into_one_category():
    """constant planes: every sample a class uses falls into category 2 with |d| = max; stripes: into the categories 0 and 4 of the classes
    that look sideways.  One 128 x 128 CTU, no neighbours: 126 x 128, 128 x 126 and 126 x 126 samples per class."""
    w = h = 128
    for bd in (8, 10):
        mx = (1 << bd) - 1
        for kind in cases.SAO_ONE_CATEGORY_KINDS:
            org, rec = cases.sao_one_category_planes(kind, w, h, bd)
            st = np.zeros((1, 5, 2, 32), np.int64)
            oracle().orc_sao_stats(p(org), w, p(rec), w, w, h, 128, 128, bd, None, 5, 4, p(st))
            n = [126 * 128, 128 * 126, 126 * 126, 126 * 126]
            for t in range(4):
                cnt, dif = st[0, t, 1, :5], st[0, t, 0, :5]
                if kind == "stripes" and t != 1:
                    assert cnt[1] == cnt[2] == cnt[3] == 0 and cnt[0] + cnt[4] == n[t] and cnt[0] == cnt[4]
                    assert dif[0] == cnt[0] * mx and dif[4] == cnt[4] * (mx - 1)
                else:
                    assert cnt[2] == n[t] and cnt.sum() == n[t]
                    assert abs(int(dif[2])) == n[t] * mx - (n[t] // 2 if kind == "stripes" else 0)
    # the packed accumulator of the scalar body (count << 21 | sum of (d + 1024)): 64 lanes x 16 rows at d = 1023
    assert 64 * 16 * 2047 == 2096128 == (1 << 21) - 1024


def test_threshold_sweep_has_residuals_that_f16_cannot_hold():
    """the single-sample sweep of test_resi_chain_single_sample_across_the_threshold: +-1023 stays on the matrix cores, +-1024 leaves them but would still
    be exact there; 16392 / -16408 would NOT: with the residual rounded to f16, as a body that missed its vote would see it, the oracle's levels of (nearly)
    every such TU change -- so a missed vote cannot pass"""
    from test_gpu_resichain import oracle_chain, threshold_case
    org, pred, tus, W, touched = threshold_case(np.random.default_rng(1024))
    r = org.astype(np.int32) - pred
    assert {int(v) for v in np.unique(r[np.abs(r) > 20])} == {1023, -1023, 1024, -1024, 16392, -16408}
    org16 = (pred + r.astype(np.float16).astype(np.int32)).astype(np.int16)
    assert int((org16 != org).sum()) == int((np.abs(r) > 2048).sum())
    lv, _, _, coffs = oracle_chain(org, pred, tus, 10, W)
    lv16 = oracle_chain(org16, pred, tus, 10, W)[0]
    seen, changed = {}, {}
    for i in touched:
        x, y, w, h = tus[i][:4]
        if min(w, h) >= 4 and max(w, h) >= 16 and int(np.abs(r[y:y + h, x:x + w]).max()) > 2048:
            seen[(w, h)] = seen.get((w, h), 0) + 1
            changed[(w, h)] = changed.get((w, h), 0) + (not np.array_equal(lv[coffs[i]:coffs[i] + w * h], lv16[coffs[i]:coffs[i] + w * h]))
    assert len(seen) == 21                                   # nine matrix-core shapes, twelve packed-tile shapes
    assert all(changed[k] >= seen[k] - 2 and changed[k] >= 10 for k in seen), (seen, changed)
