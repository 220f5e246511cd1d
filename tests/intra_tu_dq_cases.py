"""The pixel pass of the intra RD loop under DepQuant 1 (IntraSearch::xIntraCodingTUBlock, IntraSearch.cpp:1147-1316, with transformNxN / invTransformNxN going
through DQIntern::DepQuant) restated for the tests of vvcgpu_intra_tu_code_dq_batch from steps that are each pinned to the compiled reference: resolve and
predict of tests/intra_tu_code_cases.py for the mode and the prediction; the chain steps of tests/rd_pass_kit.py (subtract, forward transform, de-quantise with
dep_quant = 1 and inverse transform) with orc_depquant between them, i.e. code_slot of tests/inter_resi_dq_cases.py; reconstruct and SSE of the kit; num_sig
counted in numpy.  The item rules of this entry (level offset a multiple of 16 and not negative, levels inside the extent, rate index, lambda) are written here
from the entry's contract.  Planes, PUs, items and canaries are those of the sibling's cases; this file adds the record beside each item (lambda, rate table,
luma), level offsets in multiples of 16 and the rate tables.  numpy only: the generator and the CPU tests load this file without torch."""
import os

import numpy as np

import inter_resi_dq_cases as dqc
import intra_mode_cand_cases as imc
import intra_tu_code_cases as itc
import rd_pass_kit as kit
from vvcsoftware_vtm_amd import abi

DQ, RATES, Q_DEPQUANT = abi.INTER_RESI_DQ, abi.DQ_RATES, abi.INTRA_TU_Q_DEPQUANT
PRED_GIVEN, FROM_LIST, WRITE_PRED, NO_SMOOTHING = itc.PRED_GIVEN, itc.FROM_LIST, itc.WRITE_PRED, itc.NO_SMOOTHING
U32_MAX, U64_MAX = kit.U32_MAX, kit.U64_MAX
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "intra_tu_dq.npz")
shared_rates, last_threshold, all_shapes = dqc.shared_rates, dqc.last_threshold, imc.all_shapes


class Case:
    """tc: the sibling's TuCase (its level offsets in multiples of 16); dq: one INTER_RESI_DQ record per item; rates: the DQ_RATES array"""
    def __init__(self, tc, dq, rates):
        self.tc, self.dq, self.rates, self.bd = tc, dq, rates, tc.bd

    def sub(self, idx):
        """the case of the items idx, in that order, over the same buffers"""
        tc = self.tc
        return Case(itc.TuCase(tc.base, tc.items[idx].copy(), tc.pred0, tc.rec_size, tc.level_size), self.dq[idx].copy(), self.rates)


def resolve(case, i, flags, mode_list, have_pred=True):
    """-> (mode, filter) of item i, mode PRED_GIVEN included, or None: skipped"""
    it, q = case.tc.items[i], case.dq[i]
    lo, sz = int(it["level_off"]), int(it["w"]) * int(it["h"])
    if lo < 0 or lo % 16 or not 0 <= int(q["rates_idx"]) < len(case.rates) or not float(q["lambda"]) > 0:
        return None
    r = itc.resolve(case.tc, i, flags, mode_list, have_pred)
    if r is None or lo + sz > case.tc.level_size:
        return None
    return r


def code_block(org, pred, bd, tr_hor, tr_ver, qp, lam, luma, rates_row, clp):
    """one TU from contiguous h x w original and prediction -> (levels [h][w] int32, abs_sum, rec [h][w] int16, dist)"""
    org, pred = np.ascontiguousarray(org, np.int16), np.ascontiguousarray(pred, np.int16)
    level, abs_sum, resi2 = dqc.code_slot(kit.subtract(org, pred, bd), bd, tr_hor + 3 * tr_ver, qp, lam, luma, rates_row)
    rec = kit.reconstruct(pred, resi2, clp)
    return level, abs_sum, rec, kit.sse(org, rec)


def restate(case, flags=0, clp=None, mode_list=None, have_pred=True):
    """the entry over every item -> the dict of the sibling's restate"""
    tc = case.tc
    clp = clp or (0, (1 << tc.bd) - 1)
    n = len(tc.items)
    pred_b, rec_b, level_b = tc.initial()
    out = dict(pred=pred_b, rec=rec_b, level=level_b, abs_sum=np.full(n, U32_MAX, np.uint32), num_sig=np.full(n, U32_MAX, np.uint32),
               dist=np.full(n, U64_MAX, np.uint64), mode_out=np.full(n, -1, np.int32))
    for i, it in enumerate(tc.items):
        r = resolve(case, i, flags, mode_list, have_pred)
        if r is None:
            continue
        mode, filt = r
        q = case.dq[i]
        u = tc.base.pus[int(it["pu"])]
        w, h = int(it["w"]), int(it["h"])
        org = tc.base.org[int(u["y"]):int(u["y"]) + h, int(u["x"]):int(u["x"]) + w]
        if mode == PRED_GIVEN:
            pred = itc.block(tc.pred0, int(it["pred_off"]), int(it["pred_stride"]), w, h).copy()
        else:
            pred = itc.predict(tc.refs_of(int(it["pu"])), w, h, mode, filt, clp)
            out["mode_out"][i] = mode
            if flags & WRITE_PRED:
                itc.block(pred_b, int(it["pred_off"]), int(it["pred_stride"]), w, h)[:] = pred
        level, abs_sum, rec, dist = code_block(org, pred, tc.bd, int(it["tr_hor"]), int(it["tr_ver"]), int(it["qp"]), float(q["lambda"]), int(q["luma"]),
                                               case.rates[int(q["rates_idx"]):], clp)
        level_b[int(it["level_off"]):int(it["level_off"]) + w * h] = level.reshape(-1)
        itc.block(rec_b, int(it["rec_off"]), int(it["rec_stride"]), w, h)[:] = rec
        out["abs_sum"][i], out["num_sig"][i], out["dist"][i] = abs_sum, int(np.count_nonzero(level)), dist
    return out


# ---- builders --------------------------------------------------------------------------------------------------------------------------------------
OWN_KEYS = ("lam", "luma", "rates_idx", "level_misalign", "level_beyond")


def lambda_of(qp, bd):
    """a lambda that follows the QP: 0.57 * 2^((qp8 - 12) / 3) of the 8-bit QP, the encoder's order of magnitude (as the inter sibling's cases)"""
    return 0.57 * 2.0 ** ((qp - 6 * (bd - 8) - 12) / 3.0)


def attach(tc, specs, rates=None):
    """level offsets in multiples of 16 (every item a region of its own, canaries between) and a dq record per item.  specs may carry lam, luma, rates_idx
    (defaults: lambda_of the item's QP, luma, table i mod len(rates)), level_misalign (added to the offset) and level_beyond (the item's levels end 16
    beyond the extent)"""
    rates = shared_rates() if rates is None else rates
    dq = np.zeros(len(specs), DQ)
    lo = 16
    for i, s in enumerate(specs):
        it = tc.items[i]
        ew, eh = max(1, min(abs(int(it["w"])), 64)), max(1, min(abs(int(it["h"])), 64))
        it["level_off"] = lo + s.get("level_misalign", 0)
        lo += (ew * eh + 16 * (i % 3) + 15) // 16 * 16
        dq[i]["lambda"], dq[i]["rates_idx"], dq[i]["luma"] = s.get("lam", lambda_of(int(it["qp"]), tc.bd)), s.get("rates_idx", i % len(rates)), s.get("luma", 1)
    tc.level_size = lo + 16
    for i, s in enumerate(specs):
        if s.get("level_beyond"):
            tc.items[i]["level_off"] = tc.level_size - int(tc.items[i]["w"]) * int(tc.items[i]["h"]) + 16
            assert tc.items[i]["level_off"] >= 0 and tc.items[i]["level_off"] % 16 == 0
    return Case(tc, dq, rates)


def make(base, specs, rng, odd=False, givens=None, rates=None):
    """the sibling's make() + attach()"""
    return attach(itc.make(base, [{k: v for k, v in s.items() if k not in OWN_KEYS} for s in specs], rng, odd, givens), specs, rates)


def odd_base(rng, bd, shapes):
    """one PU per shape at an odd picture position (x and y), outside the flat patch"""
    rec, org = imc.fresh_planes(rng, bd)
    blocks = []
    for (w, h) in shapes:
        x, y = imc.place(rng, w, h)
        blocks.append((x + 1, y + 1, w, h))
    return itc.plain_case(bd, rec, org, blocks, rng)


def shapes_case(bd):
    """every one of the 25 shapes once at an odd picture position and odd strides of prediction and reconstruction, one mode each from a spread of
    planar / DC / angular modes, some from filtered references -> (Case, restatement)"""
    rng = np.random.default_rng(9900 + bd)
    shapes = all_shapes()
    base = odd_base(rng, bd, shapes)
    specs = []
    for q, (w, h) in enumerate(shapes):
        mode = itc.MODES[q % len(itc.MODES)]
        specs.append(dict(pu=q, mode=mode, filt=int(imc.use_filtered(w, h, mode)) if q % 3 else q % 2, qp=(22, 27, 32, 37)[q % 4] + 6 * (bd - 8), luma=1 - (q % 5 == 4)))
    case = make(base, specs, rng, odd=True)
    it = case.tc.items
    assert (base.pus["x"] % 2 == 1).all() and (it["pred_stride"] % 2 == 1).all() and (it["rec_stride"] % 2 == 1).all() and set(it["filt"]) == {0, 1}
    assert {(int(w), int(h)) for w, h in zip(it["w"], it["h"])} == set(shapes) and len(it) == 25
    want = restate(case)
    assert (want["abs_sum"] != U32_MAX).all()
    return case, want


SKIP_KINDS = ("w2", "w3", "w128", "pair_w", "pair_h", "mode_high", "tr_on_64", "list_slot_beyond", "list_null_row", "level_misalign4", "level_misalign8",
              "level_beyond", "rates_high", "rates_negative", "lambda_zero")


def random_lists(n_rows=6):
    """mode lists in the layout of list_out of vvcgpu_intra_mode_cand_batch: row r holds r + 1 modes (row 0: one, .. row 4: five), the last row is a null
    row (size 0)"""
    lists = np.full((n_rows, 16), -1, np.int32)
    for r in range(n_rows - 1):
        lists[r, 0] = r + 1
        lists[r, 5:5 + r + 1] = [(7 * r + 11 * k + 2) % 67 for k in range(r + 1)]
    lists[n_rows - 1, 0] = 0
    return lists


def random_case(bd, n=300):
    """mixed shapes, all nine transform pairs where the sides allow; explicit, FROM_LIST and PRED_GIVEN items; every skip kind interleaved between valid
    neighbours -> (Case, mode lists, restatement)"""
    rng = np.random.default_rng(9930 + bd)
    shapes = all_shapes()
    pu_shapes = [shapes[(7 * q + q // 25) % 25] for q in range(50)]
    base = itc.fresh_base(rng, bd, pu_shapes)
    lists = random_lists()
    specs, kinds = [], []
    for i in range(n):
        q = (i * 13 + i // 50) % len(pu_shapes)
        w, h = pu_shapes[q]
        th, tv = (int(rng.integers(0, 3)) if w <= 32 else 0), (int(rng.integers(0, 3)) if h <= 32 else 0)
        s = dict(pu=q, mode=int(rng.integers(0, 67)), tr_hor=th, tr_ver=tv, qp=int(rng.integers(20, 36)) + 6 * (bd - 8), luma=int(rng.integers(0, 2)),
                 lam=float(rng.uniform(5, 400)), intra=i % 2, sbh=(i // 2) % 2)
        s["filt"] = int(imc.use_filtered(w, h, s["mode"])) if i % 4 else i % 8 // 4
        if i % 5 == 2:
            s.update(mode=FROM_LIST, row=(i // 5) % 5, slot=0 if i % 3 else (i // 5) % 5 % (1 + (i // 5) % 5))
        elif i % 5 == 4:
            s.update(mode=PRED_GIVEN)
        kind = None
        if i % 11 == 7:
            kind = SKIP_KINDS[(i // 11) % len(SKIP_KINDS)]
            if kind == "w2": s["w"] = 2
            elif kind == "w3": s["w"] = 3
            elif kind == "w128": s["w"] = 128
            elif kind == "pair_w": s["w"] = 2 * w if w < 64 else 32
            elif kind == "pair_h": s["h"] = 2 * h if h < 64 else 32
            elif kind == "mode_high": s["mode"] = 67
            elif kind == "tr_on_64":
                q = pu_shapes.index((64, 16))
                s.update(pu=q, tr_hor=1, tr_ver=0)
            elif kind == "list_slot_beyond": s.update(mode=FROM_LIST, row=1, slot=2)
            elif kind == "list_null_row": s.update(mode=FROM_LIST, row=5, slot=0)
            elif kind == "level_misalign4": s["level_misalign"] = 4
            elif kind == "level_misalign8": s["level_misalign"] = 8
            elif kind == "level_beyond": s["level_beyond"] = True
            elif kind == "rates_high": s["rates_idx"] = 8
            elif kind == "rates_negative": s["rates_idx"] = -1
            elif kind == "lambda_zero": s["lam"] = 0.0
        specs.append(s)
        kinds.append(kind)
    case = make(base, specs, rng)
    want = restate(case, mode_list=lists)
    check_random(case, kinds, want)
    return case, lists, want


def check_random(case, kinds, want):
    """every skip kind occurs and is skipped between served neighbours, more than 250 items are served, at least a third of them with abs_sum > 0, every
    transform pair and all three mode kinds are served"""
    served = want["abs_sum"] != U32_MAX
    it = case.tc.items
    assert {k for k in kinds if k} == set(SKIP_KINDS)
    for i, k in enumerate(kinds):
        if k:
            assert not served[i] and served[i - 1] and served[i + 1], (i, k)
    assert served.sum() > 250 and (served & (want["abs_sum"] > 0)).sum() * 3 >= served.sum()
    assert {(int(a), int(b)) for a, b in zip(it["tr_hor"][served], it["tr_ver"][served])} == {(a, b) for a in range(3) for b in range(3)}
    for m in (FROM_LIST, PRED_GIVEN):
        assert (served & (it["mode"] == m)).sum() > 20
    assert (served & (it["mode"] >= 0)).sum() > 100


def random_kinds(n=300):
    return [SKIP_KINDS[(i // 11) % len(SKIP_KINDS)] if i % 11 == 7 else None for i in range(n)]


COUNT_SHAPES = ((4, 4), (8, 8), (8, 4), (16, 8), (4, 16))


def count_case(served_items, bd=10):
    """small items of which `served_items` are served (the trellis packs sixteen records into a wavefront, 64 into a workgroup), a skipped item behind
    every third"""
    rng = np.random.default_rng(9950 + served_items)
    base = itc.fresh_base(rng, bd, list(COUNT_SHAPES))
    specs = []
    for i in range(served_items):
        q = i % len(COUNT_SHAPES)
        specs.append(dict(pu=q, mode=itc.MODES[i % len(itc.MODES)], tr_hor=i % 3, tr_ver=(i // 3) % 3, qp=27 + 6 * (bd - 8)))
        if i % 3 == 0:
            specs.append(dict(pu=q, mode=1, qp=27 + 6 * (bd - 8), **(dict(lam=0.0), dict(level_misalign=8), dict(w=2))[(i // 3) % 3]))
    case = make(base, specs, rng)
    want = restate(case)
    assert (want["abs_sum"] != U32_MAX).sum() == served_items and (want["abs_sum"] == U32_MAX).sum() == (served_items + 2) // 3
    return case, want


WAVE_SHAPES = COUNT_SHAPES + ((16, 16), (32, 32), (64, 64))
WAVES = 12                                                                   # wavefronts of a workgroup of the front and the back


def wave_of(n, cus):
    """the entry deals item j to workgroup j mod G, wavefront (j div G) mod 12 of it, G = min(n, compute units) -> the wavefront's index, per item"""
    j = np.arange(n)
    g = min(n, cus)
    return j % g * WAVES + j // g % WAVES


def waves_case(cus=256, bd=10):
    """a list long enough that every one of the twelve wavefronts of every workgroup walks at least two items: 27 items per compute unit and 88 more
    (7000 on 256 compute units), each a copy of one of 48 templates drawn at random -- the PUs of COUNT_SHAPES, a 16x16, a 32x32 and a 64x64 one with
    explicit, FROM_LIST and PRED_GIVEN modes, two given predictions more than 1023 away from the original, and nine skipped ones of different kinds --, so that the served items of a wavefront differ in number from
    its neighbours'.  The templates are restated; the expectation of the list is theirs, copied to every item's own regions, and is re-checked against the
    restatement of a sample of the list -> (Case, mode lists, expectation)"""
    rng = np.random.default_rng(9940)
    base = itc.fresh_base(rng, bd, list(WAVE_SHAPES))
    lists, n_rates, mx = random_lists(), len(shared_rates()), (1 << bd) - 1
    tspecs, tgiven = [], {}

    def add(q, **kw):
        k = len(tspecs)
        s = dict(pu=q, qp=(22, 27, 32)[k % 3] + 6 * (bd - 8), rates_idx=k % n_rates, luma=k % 2)
        s["lam"] = lambda_of(s["qp"], bd)
        s.update(kw)
        far = s.pop("far", 0)
        if s.get("mode") == PRED_GIVEN:
            u = base.pus[q]
            o = base.org[int(u["y"]):int(u["y"]) + int(u["h"]), int(u["x"]):int(u["x"]) + int(u["w"])].astype(np.int32)
            g = o + rng.integers(-12, 13, o.shape) * (1 << (bd - 8))
            tgiven[k] = (g + far if far else np.clip(g, 0, mx)).astype(np.int16)
        tspecs.append(s)

    for q, (w, h) in enumerate(WAVE_SHAPES):
        for v in range(4 if w <= 16 else 2 if w == 32 else 1):
            mode = itc.MODES[(3 * q + v) % len(itc.MODES)]
            add(q, mode=mode, filt=int(imc.use_filtered(w, h, mode)) if v % 2 else 0, tr_hor=(q + v) % 3 if w <= 32 else 0, tr_ver=v % 3 if h <= 32 else 0)
    for q in range(6):
        add(q, mode=FROM_LIST, row=q % 5, slot=(q % 5) // 2)
    for q in (0, 2, 5, 6):
        add(q, mode=PRED_GIVEN, tr_hor=q % 3, tr_ver=1)
    for q, far in ((5, -1100), (6, 1100)):                                      # a residual beyond +-1023: the integer body on the wavefront's global scratch
        add(q, mode=PRED_GIVEN, far=far)
    n_served = len(tspecs)
    for q, kw in ((0, dict(lam=0.0)), (1, dict(level_misalign=8)), (2, dict(w=2)), (3, dict(rates_idx=99)), (4, dict(mode=67)), (5, dict(mode=FROM_LIST, row=1, slot=2)),
                  (5, dict(level_misalign=4)), (1, dict(rates_idx=-1)), (0, dict(mode=FROM_LIST, row=5, slot=0))):
        add(q, **kw)
    tcase = make(base, tspecs, rng, givens=tgiven)
    twant = restate(tcase, mode_list=lists)
    tserved = twant["abs_sum"] != U32_MAX
    assert tserved[:n_served].all() and not tserved[n_served:].any() and (twant["abs_sum"][:n_served] > 0).sum() * 2 >= n_served
    for k in (n_served - 2, n_served - 1):
        a, u = tcase.tc.items[k], base.pus[tspecs[k]["pu"]]
        o = base.org[int(u["y"]):int(u["y"]) + int(u["h"]), int(u["x"]):int(u["x"]) + int(u["w"])].astype(np.int32)
        assert np.abs(o - itc.block(tcase.tc.pred0, int(a["pred_off"]), int(a["pred_stride"]), int(a["w"]), int(a["h"]))).min() > 1023 and twant["abs_sum"][k] > 0

    n = 27 * cus + 88
    tmpl = rng.integers(0, len(tspecs), n)
    case = make(base, [tspecs[t] for t in tmpl], rng, givens={j: tgiven[t] for j, t in enumerate(tmpl) if t in tgiven})
    pred_b, rec_b, level_b = case.tc.initial()
    want = dict(pred=pred_b, rec=rec_b, level=level_b, **{k: twant[k][tmpl] for k in ("abs_sum", "num_sig", "dist", "mode_out")})
    for j in np.flatnonzero(tserved[tmpl]):
        a, b = tcase.tc.items[tmpl[j]], case.tc.items[j]
        w, h = int(a["w"]), int(a["h"])
        level_b[int(b["level_off"]):int(b["level_off"]) + w * h] = twant["level"][int(a["level_off"]):int(a["level_off"]) + w * h]
        itc.block(rec_b, int(b["rec_off"]), int(b["rec_stride"]), w, h)[:] = itc.block(twant["rec"], int(a["rec_off"]), int(a["rec_stride"]), w, h)
    check_waves(case, want, cus)

    idx = np.sort(rng.choice(n, 64, replace=False))                             # the copies are what the restatement gives for the items themselves
    sub = case.sub(idx)
    sw = restate(sub, mode_list=lists)
    for k in ("abs_sum", "num_sig", "dist", "mode_out"):
        assert np.array_equal(sw[k], want[k][idx]), k
    for it in sub.tc.items[sw["abs_sum"] != U32_MAX]:
        w, h, lo = int(it["w"]), int(it["h"]), int(it["level_off"])
        assert np.array_equal(sw["level"][lo:lo + w * h], want["level"][lo:lo + w * h])
        assert np.array_equal(itc.block(sw["rec"], int(it["rec_off"]), int(it["rec_stride"]), w, h), itc.block(want["rec"], int(it["rec_off"]), int(it["rec_stride"]), w, h))
    return case, lists, want


def prefix_of(case, want, m):
    """the expectation of a call on the first m items of a case, from the expectation `want` of the whole list (without WRITE_PRED): the regions of the
    served items behind them keep their canaries"""
    _, rec0, level0 = case.tc.initial()
    out = {k: want[k][:m] for k in ("abs_sum", "num_sig", "dist", "mode_out")}
    out["pred"], rec, level = want["pred"], want["rec"].copy(), want["level"].copy()
    for j in m + np.flatnonzero(want["abs_sum"][m:] != U32_MAX):
        it = case.tc.items[j]
        w, h, lo = int(it["w"]), int(it["h"]), int(it["level_off"])
        level[lo:lo + w * h] = level0[lo:lo + w * h]
        itc.block(rec, int(it["rec_off"]), int(it["rec_stride"]), w, h)[:] = itc.block(rec0, int(it["rec_off"]), int(it["rec_stride"]), w, h)
    out["rec"], out["level"] = rec, level
    return out


def wave_lengths(cus):
    """list lengths around the two counts at which the dealing changes: one item per workgroup (the second wavefront of a workgroup starts at cus + 1),
    one per wavefront (a wavefront's second item at 12 cus + 1)"""
    return [cus - 1, cus, cus + 1, WAVES * cus - 1, WAVES * cus, WAVES * cus + 1]


def check_waves(case, want, cus):
    """every wavefront of every workgroup walks at least two items; the served items of a wavefront take at least three different numbers, up to three or
    more, at least an eighth of the items is skipped, and some wavefront skips its first item and serves a later one; every shape of WAVE_SHAPES and all three mode kinds are served"""
    n = len(case.tc.items)
    wave = wave_of(n, cus)
    served = want["abs_sum"] != U32_MAX
    assert n > 2 * WAVES * cus and np.bincount(wave, minlength=WAVES * cus).min() >= 2
    per_wave = np.bincount(wave, weights=served, minlength=WAVES * cus).astype(int)
    assert len(set(per_wave)) >= 3 and per_wave.max() >= 3 and (~served).sum() * 8 >= n
    first = np.arange(n) < WAVES * min(n, cus)
    assert np.intersect1d(wave[first & ~served], wave[~first & served]).size
    it = case.tc.items[served]
    assert {(int(w), int(h)) for w, h in zip(it["w"], it["h"])} == set(WAVE_SHAPES)
    assert (it["mode"] == FROM_LIST).any() and (it["mode"] == PRED_GIVEN).any() and (it["mode"] >= 0).any()


def all_skipped_case(bd=10):
    rng = np.random.default_rng(9960)
    base = itc.fresh_base(rng, bd, [(8, 8), (16, 16), (64, 16)])
    specs = [dict(pu=0, w=2), dict(pu=0, level_misalign=4), dict(pu=1, mode=67), dict(pu=1, rates_idx=99), dict(pu=2, tr_hor=2), dict(pu=0, mode=FROM_LIST, row=0, slot=0),
             dict(pu=1, lam=-1.0), dict(pu=2, level_beyond=True), dict(pu=0, h=16)]
    case = make(base, specs, rng)
    want = restate(case)
    assert (want["abs_sum"] == U32_MAX).all()
    return case, want


def workspace_cases(bd=10):
    """two lists for one workspace: the first holds 64x64, 64x16 and 16x64 items (zeroed high-frequency regions), the second other shapes at the same offsets"""
    out = []
    for j, shapes in enumerate([[(64, 64), (64, 16), (16, 64), (32, 32), (8, 8), (64, 64)], [(16, 16), (32, 64), (64, 32), (8, 32), (4, 4), (64, 8), (32, 32)]]):
        rng = np.random.default_rng(9970 + j)
        base = itc.fresh_base(rng, bd, shapes)
        specs = [dict(pu=q, mode=itc.MODES[(q + 3 * j) % len(itc.MODES)], qp=(22, 27)[q % 2] + 6 * (bd - 8),
                      tr_hor=q % 3 if w <= 32 else 0, tr_ver=(q + 1) % 3 if h <= 32 else 0) for q, (w, h) in enumerate(shapes)]
        case = make(base, specs, rng)
        out.append((case, restate(case)))
    return out


ZERO_SHAPES = ((4, 4), (8, 8), (16, 16), (32, 8), (64, 64), (32, 32), (4, 16), (64, 16))


def zero_case(bd):
    """all-zero items, two per shape class: PRED_GIVEN with pred == org, and a flat residual that is the largest whose coefficients stay at or under the
    trellis' last threshold (the construction of the inter sibling's zero_case: one more and the DC coefficient exceeds it)"""
    rng = np.random.default_rng(9980 + bd)
    base = itc.fresh_base(rng, bd, list(ZERO_SHAPES), random_avail=False)
    specs, givens = [], {}
    for q, (w, h) in enumerate(ZERO_SHAPES):
        u = base.pus[q]
        blk = base.org[int(u["y"]):int(u["y"]) + h, int(u["x"]):int(u["x"]) + w]
        blk[:] = np.clip(blk, 40, None)                                          # room below the original for the flat residual
        org = blk.astype(np.int32)
        under = lambda v, qp: np.abs(dqc.forward(np.full((h, w), v, np.int16), bd)).max() <= last_threshold(w, h, qp, bd)
        qp = next(c for c in range(kit.max_qp(bd), 0, -6) if under(1, c) and not under(39, c))
        v = max(v for v in range(1, 40) if under(v, qp))
        assert not under(v + 1, qp) and org.min() >= v
        givens[2 * q], givens[2 * q + 1] = org, org - v
        specs += [dict(pu=q, mode=PRED_GIVEN, qp=qp, tr_hor=2 if max(w, h) <= 32 else 0, tr_ver=1 if max(w, h) <= 32 else 0), dict(pu=q, mode=PRED_GIVEN, qp=qp)]
    case = make(base, specs, rng, givens=givens)
    want = restate(case)
    check_zero(case, want)
    return case, want


def check_zero(case, want):
    """every item is served and all-zero -- abs_sum 0, num_sig 0, rec == clip(pred), dist == SSE(org, clip(pred)) -- and every second one has a non-zero residual"""
    tc = case.tc
    assert (want["abs_sum"] == 0).all() and (want["num_sig"] == 0).all() and len(tc.items) == 2 * len(ZERO_SHAPES)
    assert (want["dist"][0::2] == 0).all() and (want["dist"][1::2] > 0).all()
    mx = (1 << tc.bd) - 1
    for i, it in enumerate(tc.items):
        w, h = int(it["w"]), int(it["h"])
        u = tc.base.pus[int(it["pu"])]
        pred = np.clip(itc.block(tc.pred0, int(it["pred_off"]), int(it["pred_stride"]), w, h), 0, mx)
        org = tc.base.org[int(u["y"]):int(u["y"]) + h, int(u["x"]):int(u["x"]) + w].astype(np.int64)
        assert np.array_equal(itc.block(want["rec"], int(it["rec_off"]), int(it["rec_stride"]), w, h), pred)
        assert int(want["dist"][i]) == int(((org - pred) ** 2).sum())
        assert not np.any(want["level"][int(it["level_off"]):int(it["level_off"]) + w * h])


CLIP_SHAPES = ((4, 4), (8, 8), (16, 16), (32, 32), (64, 64), (8, 4), (16, 4), (64, 32))


def clip_case(bd):
    """predictions AT the clip bounds with the original just inside: resi' overshoots and the reconstruction clip bites -> (Case, restatement)"""
    rng = np.random.default_rng(9990 + bd)
    mx = (1 << bd) - 1
    rec, org = imc.fresh_planes(rng, bd)
    blocks = [imc.place(rng, w, h) + (w, h) for (w, h) in CLIP_SHAPES]
    givens = {}
    for q, (x, y, w, h) in enumerate(blocks):
        near = rng.integers(0, 48 << (bd - 8), (h, w))
        org[y:y + h, x:x + w] = near if q % 2 else mx - near
        givens[q] = np.full((h, w), 0 if q % 2 else mx, np.int16)
    base = itc.plain_case(bd, rec, org, blocks)
    case = make(base, [dict(pu=q, mode=PRED_GIVEN, qp=27 + 6 * (bd - 8), lam=30.0) for q in range(len(blocks))], rng, givens=givens)
    want = restate(case)
    bites = 0
    for i, it in enumerate(case.tc.items):                                     # the clip bites: the unclipped reconstruction differs
        w, h = int(it["w"]), int(it["h"])
        level = want["level"][int(it["level_off"]):int(it["level_off"]) + w * h]
        resi2 = kit.dequant_inverse(np.ascontiguousarray(level), w, h, bd, 0, 0, int(it["qp"]), dep_quant=1)
        bites += bool(np.any((givens[i].astype(np.int32) + resi2 < 0) | (givens[i].astype(np.int32) + resi2 > mx)))
    assert bites * 2 >= len(blocks) and (want["abs_sum"] > 0).sum() * 2 >= len(blocks)
    return case, want


def with_dq(tc_want, bd):
    """a case of the sibling (its (TuCase, restatement) pair: checker, bounds_case) with the records of this entry"""
    tc = tc_want[0]
    specs = [dict() for _ in tc.items]
    case = attach(itc.TuCase(tc.base, tc.items.copy(), tc.pred0, tc.rec_size, tc.level_size), specs)
    return case, restate(case)


def chain_case(bd=10):
    """every shape once with explicit modes and given predictions, DCT-II and EMT pairs: what the seven-launch chain serves"""
    rng = np.random.default_rng(9995)
    shapes = all_shapes()
    base = itc.fresh_base(rng, bd, shapes)
    specs = []
    for q, (w, h) in enumerate(shapes):
        pairs = itc.emt_pairs(w, h)
        th, tv = pairs[q % len(pairs)]
        mode = PRED_GIVEN if q % 4 == 3 else itc.MODES[q % len(itc.MODES)]
        specs.append(dict(pu=q, mode=mode, filt=int(imc.use_filtered(w, h, max(mode, 0))), tr_hor=th, tr_ver=tv, qp=(22, 27, 32, 37)[q % 4] + 6 * (bd - 8), luma=q % 2))
    return make(base, specs, rng)


def handover_case(bd):
    """the sibling's hand-over list (PUs for vvcgpu_intra_mode_cand_batch; FROM_LIST items for slots 0 .. 3 per PU, so slots beyond a PU's list are skipped)
    -> (imc case, its restatement, Case, restatement driven by the restated lists)"""
    base, cand, tc, _ = itc.handover_case(bd)
    case = attach(tc, [dict(luma=1) for _ in tc.items])
    want = restate(case, mode_list=cand["lists"])
    skipped = want["abs_sum"] == U32_MAX
    assert (tc.items["mode"] == FROM_LIST).all() and skipped.any() and (~skipped).sum() * 2 >= len(skipped) and (want["mode_out"][~skipped] >= 0).all()
    return base, cand, case, want


# ---- the golden file -------------------------------------------------------------------------------------------------------------------------------
def golden_case(g, bd):
    k = "bd%d_" % bd
    tc, flags = itc.golden_case(g, bd)
    return Case(tc, g[k + "dq"].view(DQ).reshape(-1), g[k + "rates"].view(RATES).reshape(-1)), flags
