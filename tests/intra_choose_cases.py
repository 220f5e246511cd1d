"""vvcgpu_intra_luma_choose_batch and vvcgpu_intra_chroma_choose_batch: the restatement, the case builders, the rate items of a chroma pass and the
golden file's reader.

luma_choose is the transform loop of IntraSearch::xRecurIntraCodingLumaQT (IntraSearch.cpp:1429-1588) inside the mode loop of estIntraPredLumaQT
(:637-697), chroma_choose the mode loop of estIntraPredChromaQT (:773-847), both as ONE sequential walk per PU in the host's order over plain Python
numbers (the kernel forms the costs on its lanes first); luma_commit / chroma_commit are the copies of the winner on host arrays.
tests/golden/gen_intra_choose.py asserts that the two compares reproduce what its own walk over the compiled reference's RdCost::calcRdCost gives;
tests/golden/intra_choose.npz holds that data.  numpy only."""
import functools
import os
import sys

import numpy as np

from rd_pass_kit import block, cost_of, side_ok, weighted  # noqa: F401  (the chains and tests take them from here)
from rd_pass_kit import same as kit_same
from vvcsoftware_vtm_amd import abi
from vvcsoftware_vtm_amd.abi import (INTRA_CHOOSE_EMT_FLAG, INTRA_CHOOSE_FAST_EMT, INTRA_CHOOSE_PASSED, INTRA_CHOOSE_PU, INTRA_CHOOSE_RESULT,
                                     INTRA_CHOOSE_TS_LAST, INTRA_CHROMA_CHOOSE_PU, INTRA_CHROMA_CHOOSE_RESULT, INTRA_CHROMA_PU, RESI_RATE_CTX_BYTES,
                                     RESI_RATE_ITEM)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "intra_choose.npz")
U32_MAX, U64_MAX = 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF
DBL_MAX = sys.float_info.max
DBL_MAX_BITS = int(np.array([DBL_MAX]).view(np.uint64)[0])
EMT_SIG_NUM_THR = 2                                                         # g_EmtSigNumThr (Rom.cpp:504)
COST_CANARY = 0x7FF8DEADBEEF0001                                            # what cand_cost / slot_cost hold before a call (a NaN too, another one)
COUNTS = ("num_sig_rule", "ts_rule", "fast_emt_after_cbf0", "winner_t_above_0", "equal_costs", "slot_passed", "no_winner")
CHROMA_COUNTS = tuple("cbf_%d%d" % (a, b) for a in (0, 1) for b in (0, 1)) + tuple("winner_slot_%d" % k for k in range(6))


def bits_of(x):
    return int(np.array([x], np.float64).view(np.uint64)[0])


def empty_result(n, dtype):
    r = np.zeros(n, dtype)
    r[dtype.names[0]], r["best_mode"], r["dist"], r["bits"], r["cost"] = -1, -1, U64_MAX, U64_MAX, DBL_MAX
    if "best_tr" in dtype.names:
        r["best_tr"] = -1
    return r


# ---- luma ------------------------------------------------------------------------------------------------------------------------------------------
def luma_pu_ok(u, w, h, n):
    """the contract of a PU -> its candidate count, or 0: outside"""
    nm, nt, first = int(u["n_modes"]), int(u["n_tr"]), int(u["cand_first"])
    if not (1 <= nm <= 16 and 1 <= nt <= 5 and first >= 0 and first + nm * nt <= n and 0 <= u["flags"] <= 7 and not u["reserved"].any()):
        return 0
    sl = slice(first, first + nm * nt)
    if not (side_ok(int(w[first]), 4) and side_ok(int(h[first]), 4) and (w[sl] == w[first]).all() and (h[sl] == h[first]).all()):
        return 0
    return nm * nt


def luma_bits(u, c, j):
    cbf = int(c["abs_sum"][j]) > 0
    mode, cls = int(c["mode_out"][j]), 3
    for k in range(3):
        if mode == int(u["mpm"][k]):
            cls = k
            break
    return int(u["mode_bits"][cls]) + int(u["cbf_bits"][int(cbf)]) + (int(u["emt_cu_bits"]) + int(c["frac_bits"][j]) if cbf else 0)


def luma_choose(c, cand_cost0=None, counts=None):
    """the entry over c = dict(pus, w, h, abs_sum, num_sig, dist, mode_out, frac_bits, scale) -> dict(cand_cost uint64 [n], result)"""
    n = len(c["abs_sum"])
    out = np.full(n, COST_CANARY, np.uint64) if cand_cost0 is None else cand_cost0.copy()
    res = empty_result(len(c["pus"]), INTRA_CHOOSE_RESULT)
    note = (lambda k: None) if counts is None else (lambda k: counts.__setitem__(k, counts.get(k, 0) + 1))
    for p, u in enumerate(c["pus"]):
        if not luma_pu_ok(u, c["w"], c["h"], n):
            continue
        nm, nt, first, flags = int(u["n_modes"]), int(u["n_tr"]), int(u["cand_first"]), int(u["flags"])
        valid = lambda j: int(c["abs_sum"][j]) != U32_MAX and (int(c["abs_sum"][j]) == 0 or int(c["frac_bits"][j]) != U64_MAX)
        out[first:first + nm * nt] = INTRA_CHOOSE_PASSED
        best, best_cost = None, DBL_MAX
        for m in range(nm):
            if not valid(first + m * nt):
                note("slot_passed")
                continue
            single, bt, cbf_best = DBL_MAX, None, False
            for t in range(nt):
                j = first + m * nt + t
                ts = bool(flags & INTRA_CHOOSE_TS_LAST) and t == nt - 1
                if (flags & INTRA_CHOOSE_FAST_EMT) and t > 0 and not ts and not cbf_best:
                    if bt is not None:
                        note("fast_emt_after_cbf0")
                    continue
                if not valid(j):
                    continue
                cbf = int(c["abs_sum"][j]) > 0
                if ts and not cbf:
                    cost = DBL_MAX
                    note("ts_rule")
                elif (flags & INTRA_CHOOSE_EMT_FLAG) and t > 0 and not ts and int(c["num_sig"][j]) <= EMT_SIG_NUM_THR:
                    cost = DBL_MAX
                    note("num_sig_rule")
                else:
                    cost = cost_of(c["scale"], c["dist"][j], luma_bits(u, c, j))
                out[j] = bits_of(cost)
                if cost == single and cost != DBL_MAX:
                    note("equal_costs")
                if cost < single:
                    single, bt, cbf_best = cost, j, cbf
            if bt is not None and single == best_cost:
                note("equal_costs")
            if bt is not None and single < best_cost:
                best_cost, best = single, bt
        if best is None:
            note("no_winner")
            continue
        if (best - first) % nt:
            note("winner_t_above_0")
        r = res[p]
        r["best_cand"], r["best_mode"], r["best_tr"], r["cbf"] = best, c["mode_out"][best], (best - first) % nt, int(c["abs_sum"][best]) > 0
        r["dist"], r["bits"], r["cost"] = c["dist"][best], luma_bits(u, c, best), best_cost
    return dict(cand_cost=out, result=res)


def luma_commit(c, result, tus, rec, level, ctx_out, rec_dst, level_dst, ctx_best):
    """the copies of the winners -> (rec_dst, level_dst, ctx_best) after them (ctx_out / ctx_best may be None)"""
    rec_dst, level_dst, ctx_best = rec_dst.copy(), level_dst.copy(), None if ctx_best is None else ctx_best.copy()
    for p, (u, r) in enumerate(zip(c["pus"], result)):
        j = int(r["best_cand"])
        if j < 0:
            continue
        t = tus[j]
        w, h = int(t["w"]), int(t["h"])
        block(rec_dst, int(u["rec_dst_off"]), int(u["rec_dst_stride"]), w, h)[:] = block(rec, int(t["rec_off"]), int(t["rec_stride"]), w, h)
        level_dst[int(u["level_dst_off"]):int(u["level_dst_off"]) + w * h] = level[int(t["level_off"]):int(t["level_off"]) + w * h]
        if ctx_best is not None:
            ctx_best[p] = ctx_out[j]
    return rec_dst, level_dst, ctx_best


def random_luma(seed, n_pu, cand_of=None, bad=True, shapes=((4, 4), (8, 4), (4, 8), (8, 8), (16, 16), (32, 8), (64, 64)), cycle=False):
    """n_pu PUs with mixed n_modes / n_tr and flags; candidates skipped alone and by the slot, without a level, with too few levels, duplicated (ties);
    gaps between the PUs' ranges; with `bad` every seventh PU outside the contract in a way of its own.  cand_of(rng, w, h) -> (abs_sum, num_sig,
    frac_bits) of a served candidate (default: random numbers); cycle: PU p takes shape p mod len(shapes) -> the dict luma_choose takes"""
    rng = np.random.default_rng(seed)
    pus = np.zeros(n_pu, INTRA_CHOOSE_PU)
    w, h, abs_sum, num_sig, dist, mode_out, frac = [], [], [], [], [], [], []

    def default_cand(rng, cw, ch):
        ns = int(rng.integers(1, 7)) if rng.random() < 0.7 else int(rng.integers(7, cw * ch + 1))
        return ns + int(rng.integers(0, 40)), ns, int(rng.integers(1 << 12, 1 << 21))
    cand_of = cand_of or default_cand
    for p in range(n_pu):
        cw, ch = shapes[p % len(shapes) if cycle else int(rng.integers(0, len(shapes)))]
        nm = int(rng.integers(1, 4)) if rng.random() < 0.7 else int(rng.integers(4, 17))
        nt = int(rng.choice([1, 2, 5, 5, 3, 4]))
        flags = int(rng.integers(0, 8))
        if nt == 1 and rng.random() < 0.7:
            flags &= ~INTRA_CHOOSE_TS_LAST
        for g in range(int(rng.integers(0, 3))):                             # candidates of no PU
            w.append(cw); h.append(ch); abs_sum.append(3); num_sig.append(2); dist.append(7); mode_out.append(1); frac.append(99)
        first = len(w)
        mpm = rng.choice(67, 3, replace=False)
        pus[p]["cand_first"], pus[p]["n_modes"], pus[p]["n_tr"], pus[p]["flags"], pus[p]["mpm"] = first, nm, nt, flags, mpm
        pus[p]["mode_bits"] = rng.integers(1 << 14, 1 << 18, 4)
        pus[p]["cbf_bits"] = rng.integers(1 << 10, 1 << 17, 2)
        pus[p]["emt_cu_bits"] = int(rng.integers(1 << 10, 1 << 17)) if flags & INTRA_CHOOSE_EMT_FLAG or rng.random() < 0.3 else 0
        dead_pu = rng.random() < 0.06                                        # a PU whose every slot is passed over: no winner
        for m in range(nm):
            mode = int(mpm[int(rng.integers(0, 3))]) if rng.random() < 0.4 else int(rng.integers(0, 67))
            dead = dead_pu or rng.random() < 0.12                            # a slot beyond its list
            for t in range(nt):
                k = len(w) - first
                w.append(cw); h.append(ch); mode_out.append(mode)
                r = rng.random()
                if dead or r < 0.06:
                    abs_sum.append(U32_MAX); num_sig.append(U32_MAX); dist.append(U64_MAX); frac.append(U64_MAX); mode_out[-1] = -1
                elif k and r < 0.22:                                         # a copy of an earlier candidate of the PU: equal costs where both count
                    s = first + int(rng.integers(0, k))
                    abs_sum.append(abs_sum[s]); num_sig.append(num_sig[s]); dist.append(dist[s]); frac.append(frac[s]); mode_out[-1] = mode_out[s]
                elif r < 0.40:
                    abs_sum.append(0); num_sig.append(0); dist.append(int(rng.integers(0, 1 << 20))); frac.append(0)
                else:
                    a, ns, fb = cand_of(rng, cw, ch)
                    abs_sum.append(a); num_sig.append(ns); dist.append(int(rng.integers(0, 1 << 20))); frac.append(U64_MAX if r > 0.98 else fb)
    n = len(w)
    c = dict(pus=pus, w=np.array(w, np.int16), h=np.array(h, np.int16), abs_sum=np.array(abs_sum, np.uint32), num_sig=np.array(num_sig, np.uint32),
             dist=np.array(dist, np.uint64), mode_out=np.array(mode_out, np.int32), frac_bits=np.array(frac, np.uint64), scale=float(rng.uniform(20.0, 900.0)))
    if bad:
        kinds = [dict(n_modes=0), dict(n_modes=17), dict(n_tr=0), dict(n_tr=6), dict(cand_first=-1), dict(cand_first=n - 1), dict(flags=8),
                 dict(reserved=[0, 1]), "w_differs", "h_differs", "side_2", "side_128", "side_12"]
        for i, p in enumerate(range(3, n_pu, 7)):
            kind = kinds[i % len(kinds)]
            first, cnt = int(pus[p]["cand_first"]), int(pus[p]["n_modes"]) * int(pus[p]["n_tr"])
            if isinstance(kind, dict):
                for f, v in kind.items():
                    pus[p][f] = v
                if "cand_first" in kind and kind["cand_first"] == n - 1 and cnt == 1:
                    pus[p]["n_modes"] = 2
            elif kind == "w_differs":
                c["w"][first + cnt - 1] *= 2
            elif kind == "h_differs":
                c["h"][first + cnt - 1] = 4 if c["h"][first] != 4 else 8
            else:
                c["w"][first:first + cnt] = int(kind[5:])
    return c


def luma_tus(c, rng=None, odd=False):
    """candidate buffers for the commit: an RC_DESC per candidate with a reconstruction block (rec_stride == w, or larger on every other candidate) and a
    level block of its own -> (tus, rec int16, level int32), both buffers random"""
    rng = rng or np.random.default_rng(1)
    n = len(c["w"])
    tus = np.zeros(n, abi.RC_DESC)
    ro, lo = (3 if odd else 4), 4
    for j in range(n):
        w, h = int(c["w"][j]), int(c["h"][j])
        ew, eh = max(1, min(abs(w), 64)), max(1, min(abs(h), 64))
        rs = ew + (0 if j % 2 == 0 else (3 if odd else 8))
        tus[j]["w"], tus[j]["h"], tus[j]["rec_off"], tus[j]["rec_stride"], tus[j]["level_off"] = w, h, ro, rs, lo
        ro += eh * rs + (1 + j % 3 if odd else 4)
        lo += ew * eh + 4 * (j % 2)
    return tus, rng.integers(0, 1024, ro + 8).astype(np.int16), rng.integers(-300, 301, lo + 8).astype(np.int32)


def place_luma_dst(c, rng, stride=204, unit=4):
    """destination blocks for the PUs in a plane `stride` samples wide: a band per PU, x an odd multiple of `unit`; fills rec_dst_off / rec_dst_stride /
    level_dst_off -> (plane size, level store size)"""
    y, lo = 1, unit
    for p, u in enumerate(c["pus"]):
        first = min(max(int(u["cand_first"]), 0), len(c["w"]) - 1)
        w, h = max(1, min(abs(int(c["w"][first])), 64)), max(1, min(abs(int(c["h"][first])), 64))
        x = unit * (2 * int(rng.integers(0, (stride - w) // (2 * unit))) + 1)
        u["rec_dst_off"], u["rec_dst_stride"], u["level_dst_off"] = y * stride + x, stride, lo
        y += h + 1
        lo += w * h + (4, 2, 1, 3)[p % 4]                                   # level blocks at every alignment
    return (y + 1) * stride, lo + 8


# ---- chroma ----------------------------------------------------------------------------------------------------------------------------------------
def chroma_choose(c, slot_cost0=None, counts=None):
    """the entry over c = dict(cpus, pus, abs_sum [n][6][2], dist [n][6][2], frac_cb, frac_cr [12 n], scale) -> dict(slot_cost uint64 [n][6], result)"""
    n = len(c["pus"])
    out = np.full((n, 6), COST_CANARY, np.uint64) if slot_cost0 is None else slot_cost0.copy()
    res = empty_result(n, INTRA_CHROMA_CHOOSE_RESULT)
    a, d = c["abs_sum"].reshape(n, 6, 2), c["dist"].reshape(n, 6, 2)
    fcb, fcr = c["frac_cb"].reshape(n, 6, 2)[:, :, 0], c["frac_cr"].reshape(n, 6, 2)[:, :, 1]
    note = (lambda k: None) if counts is None else (lambda k: counts.__setitem__(k, counts.get(k, 0) + 1))
    for p, (u, q) in enumerate(zip(c["cpus"], c["pus"])):
        out[p] = INTRA_CHOOSE_PASSED
        if not (side_ok(int(q["w"]), 2) and side_ok(int(q["h"]), 2)) or u["reserved"].any():
            continue
        best, best_cost = None, DBL_MAX
        for k in range(6):
            s = [int(a[p, k, 0]), int(a[p, k, 1])]
            cbf = [s[0] > 0, s[1] > 0]
            if int(q["mode"][k]) == -1 or U32_MAX in s or (cbf[0] and int(fcb[p, k]) == U64_MAX) or (cbf[1] and int(fcr[p, k]) == U64_MAX):
                continue
            bits = int(u["mode_bits"][k]) + int(u["cbf_cb_bits"][int(cbf[0])]) + int(u["cbf_cr_bits"][2 * int(cbf[0]) + int(cbf[1])])
            bits += (int(fcb[p, k]) if cbf[0] else 0) + (int(fcr[p, k]) if cbf[1] else 0)
            dist = weighted(u["dist_weight"][0], d[p, k, 0]) + weighted(u["dist_weight"][1], d[p, k, 1])
            cost = cost_of(c["scale"], dist, bits)
            out[p, k] = bits_of(cost)
            note("cbf_%d%d" % (cbf[0], cbf[1]))
            if cost < best_cost:
                best_cost, best = cost, (k, cbf, dist, bits)
        if best is None:
            continue
        note("winner_slot_%d" % best[0])
        r = res[p]
        r["best_slot"], r["best_mode"], r["cbf"], r["dist"], r["bits"], r["cost"] = best[0], q["mode"][best[0]], best[1], best[2], best[3], best_cost
    return dict(slot_cost=out, result=res)


def chroma_commit(c, result, cand_rec, level, ctx_out, rec_dst, level_dst, ctx_best):
    """the copies of the winners, both components -> (rec_dst, level_dst, ctx_best) after them"""
    rec_dst, level_dst, ctx_best = rec_dst.copy(), level_dst.copy(), None if ctx_best is None else ctx_best.copy()
    for p, (u, q, r) in enumerate(zip(c["cpus"], c["pus"], result)):
        k = int(r["best_slot"])
        if k < 0:
            continue
        w, h = int(q["w"]), int(q["h"])
        for comp in range(2):
            so, lo = int(q["cand_off"]) + (2 * k + comp) * w * h, int(q["level_off"]) + (2 * k + comp) * w * h
            block(rec_dst, int(u["rec_dst_off"][comp]), int(u["rec_dst_stride"]), w, h)[:] = block(cand_rec, so, w, w, h)
            level_dst[int(u["level_dst_off"][comp]):int(u["level_dst_off"][comp]) + w * h] = level[lo:lo + w * h]
        if ctx_best is not None:
            ctx_best[p] = ctx_out[12 * p + 2 * k + 1]
    return rec_dst, level_dst, ctx_best


def chroma_rate_items(pus, dep_quant, ctx_idx=0):
    """the item lists of the two vvcgpu_resi_rate_batch calls behind a chroma pass, 12 n items each at 12 p + 2 k + c: the Cb blocks from row ctx_idx
    of the contexts (ctxStart), then the Cr blocks from row 12 p + 2 k of the first call's ctx_out; the other component's items carry w = 0 and are
    skipped.  Both calls take gate = the pass' abs_sum -> (items_cb, items_cr)"""
    n = len(pus)
    area = pus["w"].astype(np.int64) * pus["h"]
    out = []
    for comp in range(2):
        it = np.zeros((n, 6, 2), RESI_RATE_ITEM)
        it["ts_flag"], it["emt_idx"] = -1, -1
        v = it[:, :, comp]
        v["level_off"] = pus["level_off"][:, None] + (2 * np.arange(6)[None] + comp) * area[:, None]
        v["w"], v["h"], v["dep_quant"] = pus["w"][:, None], pus["h"][:, None], dep_quant
        v["sign_hiding"] = 0 if dep_quant else pus["sign_hiding"][:, None]
        v["ctx_idx"] = ctx_idx if comp == 0 else 12 * np.arange(n)[:, None] + 2 * np.arange(6)[None]
        out.append(it.reshape(-1))
    return out[0], out[1]


def random_chroma(seed, n, shapes=((2, 2), (2, 8), (8, 2), (4, 4), (8, 8), (16, 4), (32, 32), (64, 64)), bad=True, cycle=False):
    """n chroma PUs: unused slots, slots with markers, every (cbf_cb, cbf_cr) pair, duplicated slots (ties), both weights; with `bad` every ninth PU
    outside the contract -> the dict chroma_choose takes (cand_off / level_off of the PUs laid out one behind the other)"""
    rng = np.random.default_rng(seed)
    cpus, pus = np.zeros(n, INTRA_CHROMA_CHOOSE_PU), np.zeros(n, INTRA_CHROMA_PU)
    abs_sum = rng.integers(1, 60, (n, 6, 2)).astype(np.uint32) * (rng.random((n, 6, 2)) < 0.6)
    dist = rng.integers(0, 1 << 19, (n, 6, 2)).astype(np.uint64)
    fcb, fcr = (rng.integers(1 << 12, 1 << 20, (n, 6, 2)).astype(np.uint64) for _ in range(2))
    off = 4
    for p in range(n):
        w, h = shapes[p % len(shapes) if cycle else int(rng.integers(0, len(shapes)))]
        pus[p]["w"], pus[p]["h"], pus[p]["cand_off"], pus[p]["level_off"] = w, h, off, off
        off += 12 * w * h + 4 * (p % 3)
        modes = [int(rng.integers(0, 68)) for _ in range(6)]
        for k in range(6):
            r = rng.random()
            if r < 0.15:
                modes[k] = -1
            if r < 0.25:
                abs_sum[p, k] = U32_MAX
                dist[p, k] = U64_MAX
            elif k and r < 0.4:
                s = int(rng.integers(0, k))
                abs_sum[p, k], dist[p, k], fcb[p, k], fcr[p, k] = abs_sum[p, s], dist[p, s], fcb[p, s], fcr[p, s]
            elif r > 0.97:
                fcr[p, k, 1] = U64_MAX
        pus[p]["mode"] = modes
        cpus[p]["mode_bits"] = rng.integers(1 << 13, 1 << 17)                # one value: duplicated slots tie
        cpus[p]["mode_bits"][int(rng.integers(0, 6))] += int(rng.integers(0, 3))
        cpus[p]["cbf_cb_bits"], cpus[p]["cbf_cr_bits"] = rng.integers(1 << 10, 1 << 17, 2), rng.integers(1 << 10, 1 << 17, 4)
        cpus[p]["dist_weight"] = (1.0, 1.0) if rng.random() < 0.3 else rng.uniform(0.6, 1.9, 2)
    if bad:
        for i, p in enumerate(range(4, n, 9)):
            if i % 3 == 0:
                pus[p]["w"] = (1, 128, 12)[(i // 3) % 3]
            elif i % 3 == 1:
                pus[p]["h"] = (0, 3)[(i // 3) % 2]
            else:
                cpus[p]["reserved"][i % 3] = 1
    fcb[abs_sum == U32_MAX], fcr[abs_sum == U32_MAX] = U64_MAX, U64_MAX
    return dict(cpus=cpus, pus=pus, abs_sum=abs_sum, dist=dist, frac_cb=fcb.reshape(-1), frac_cr=fcr.reshape(-1), scale=float(rng.uniform(20.0, 900.0)),
                cand_size=off + 8)


def place_chroma_dst(c, rng, stride=106, unit=2):
    """destination blocks of both components in a plane `stride` samples wide (Cb bands above, Cr bands below), x an odd multiple of `unit`
    -> (plane size, level store size)"""
    y, lo = 1, unit
    for comp in range(2):
        for p, (u, q) in enumerate(zip(c["cpus"], c["pus"])):
            w, h = max(1, min(abs(int(q["w"])), 64)), max(1, min(abs(int(q["h"])), 64))
            x = unit * (2 * int(rng.integers(0, (stride - w) // (2 * unit))) + 1)
            u["rec_dst_off"][comp], u["rec_dst_stride"], u["level_dst_off"][comp] = y * stride + x, stride, lo
            y += h + 1
            lo += w * h + (4, 2, 1, 3)[p % 4]                                   # level blocks at every alignment
    return (y + 1) * stride, lo + 8


# ---- the golden file -------------------------------------------------------------------------------------------------------------------------------
def golden():
    return np.load(GOLDEN, allow_pickle=False)


def golden_luma(g):
    c = {k: g["luma_" + k] for k in ("w", "h", "abs_sum", "num_sig", "dist", "mode_out", "frac_bits")}
    c["pus"] = np.ascontiguousarray(g["luma_pus"]).view(INTRA_CHOOSE_PU).reshape(-1)
    c["scale"] = float(g["luma_scale"].view(np.float64)[0])
    want = dict(cand_cost=g["luma_cand_cost"], result=np.ascontiguousarray(g["luma_result"]).view(INTRA_CHOOSE_RESULT).reshape(-1))
    return c, want


def golden_chroma(g):
    c = {k: g["chroma_" + k] for k in ("abs_sum", "dist", "frac_cb", "frac_cr")}
    c["cpus"] = np.ascontiguousarray(g["chroma_cpus"]).view(INTRA_CHROMA_CHOOSE_PU).reshape(-1)
    c["pus"] = np.ascontiguousarray(g["chroma_pus"]).view(INTRA_CHROMA_PU).reshape(-1)
    c["scale"] = float(g["chroma_scale"].view(np.float64)[0])
    want = dict(slot_cost=g["chroma_slot_cost"], result=np.ascontiguousarray(g["chroma_result"]).view(INTRA_CHROMA_CHOOSE_RESULT).reshape(-1))
    return c, want


same = functools.partial(kit_same, bytewise=True)                            # the costs are compared as 64 bits: the marker is a NaN

assert RESI_RATE_CTX_BYTES == 192
