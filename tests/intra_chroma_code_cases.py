"""The pixel work of the intra chroma mode loop (IntraSearch::estIntraPredChromaQT, IntraSearch.cpp:704-852: xIntraCodingTUBlock for Cb and Cr per candidate
mode) restated for the tests of vvcgpu_intra_chroma_code_batch from oracle steps that are each pinned to the compiled reference: orc_intra_fill_refs
(tests/golden/intra_fill.npz), orc_intra_pred -- the restated predIntraAng, which runs 2-sample sides through the same code; tests/golden/gen_intra_chroma_code.py
proves those against the reference's own predIntraAng --, orc_cclm_pred (tests/golden/cclm.npz) with the chroma neighbours taken from row 0 / column 0 of the
references, and the chain steps of tests/rd_pass_kit.py as intra_tu_code_cases.code_block composes them.  The contract (which PU is served, which slot) is written here from include/vvcgpu.h.
Also the case builders: a luma reconstruction, a chroma reconstruction and a chroma original of one 4:2:0 picture, PUs grouped by shape with candidate buffers
of their own and canaries between them.  numpy only: the generator and the CPU tests load this file without torch."""
import ctypes as C
import os

import numpy as np

import intra_mode_cand_cases as imc
import intra_tu_code_cases as itc
import pu_search_kit as kit
import rd_pass_kit as rd
from oraclelib import oracle, p
from vvcsoftware_vtm_amd import abi

LM, WRITE_PRED = abi.INTRA_CHROMA_LM, abi.INTRA_CHROMA_WRITE_PRED
SLOTS = 6
CW, CH = 104, 88                    # the chroma planes; the luma plane is twice that
UNIT = 2                            # pcv.minCUWidth / Height (4) shifted by the chroma scale
U32_MAX, U64_MAX = rd.U32_MAX, rd.U64_MAX
PRED_CANARY, REC_CANARY, LEVEL_CANARY, REFS_CANARY = rd.PRED_CANARY, rd.REC_CANARY, rd.LEVEL_CANARY, rd.REFS_CANARY
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "intra_chroma_code.npz")
SHAPES = [(2, 2), (2, 8), (8, 2), (4, 4), (8, 8), (4, 16), (16, 16), (32, 8), (32, 32), (64, 64), (64, 16)]
ref_lengths, ilog2, wide_angle = imc.ref_lengths, imc.ilog2, imc.wide_angle


def cand_modes(dm, lm=True):
    """PU::getIntraChromaCandModes (UnitTools.cpp:466-491) with DM resolved: planar, vertical, horizontal, DC with VDIA in place of the one that equals the
    luma mode, then LM (or unused), then DM"""
    return [66 if m == dm else m for m in (0, 50, 18, 1)] + [LM if lm else -1, dm]


def n_units(w, h, unit=UNIT):
    return imc.n_units(w, h, unit)


def planes(rng, bd):
    """-> (luma reconstruction [2 CH][2 CW], chroma reconstruction [2][CH][CW], chroma original [2][CH][CW]); the chroma follows the luma, so that the
    linear model has something to find"""
    mx = (1 << bd) - 1
    luma = kit.texture(rng, 2 * CH, 2 * CW, bd, 0.0)
    ds = luma[::2, ::2].astype(np.float64)
    rec = np.stack([np.clip(np.rint(0.2 * mx + 0.55 * ds + rng.normal(0, mx / 150.0, ds.shape)), 0, mx),
                    np.clip(np.rint(0.8 * mx - 0.45 * ds + rng.normal(0, mx / 150.0, ds.shape)), 0, mx)]).astype(np.int16)
    org = np.clip(np.roll(rec, (1, -1), axis=(1, 2)).astype(np.int32) + rng.integers(-3, 4, rec.shape) * (1 << (bd - 8)), 0, mx).astype(np.int16)
    return luma, rec, org


def availability(w, h, x, y, kind, rng=None):
    """neighborFlags of a chroma block at (x, y), one byte per 2-sample unit in chain order.  kind: 'all', 'none', 'random', or a pair (above, left) --
    that side's units (with the above-right / below-left ones, and the top-left unless both are 1) all set or all cleared.  A unit outside the plane is
    never available."""
    T, L = ref_lengths(w, h)
    above, left = (T + UNIT - 1) // UNIT, (L + UNIT - 1) // UNIT
    f = np.ones(above + left + 1, np.uint8)
    if kind == "none":
        f[:] = 0
    elif kind == "random":
        f = np.repeat(rng.integers(0, 2, f.size).astype(np.uint8), int(rng.integers(1, 4)))[:f.size].copy()
    elif kind != "all":
        a, l = kind
        f[left + 1:] = a
        f[:left] = l
        f[left] = a and l
    for u in range(left):                                   # chain order runs upwards: unit u covers rows (left - u) UNIT - UNIT .. - 1 below y
        if y + (left - u) * UNIT > CH or x < 1:
            f[u] = 0
    if x < 1 or y < 1:
        f[left] = 0
    for u in range(above):
        if x + (u + 1) * UNIT > CW or y < 1:
            f[left + 1 + u] = 0
    return f


def cclm_flags(f, w, h):
    """the reference's bAboveAvaillable / bLeftAvaillable (:1633-1637): ALL units of that side of the block"""
    L = ref_lengths(w, h)[1]
    left = (L + UNIT - 1) // UNIT
    nl, na = max(1, h // UNIT), max(1, w // UNIT)
    return int(f[left + 1:left + 1 + na].all()), int(f[left - nl:left].all())


class Case:
    """luma, rec, org: the planes; avail: the flags of every PU; pus (abi.INTRA_CHROMA_PU), fill (abi.INTRA_FILL_DESC, two per PU) and runs ((w, h, count)
    triples) exactly as the entry takes them; the sizes of the reference buffer and of the candidate buffers"""
    def __init__(self, bd, luma, rec, org, avail, pus, fill, runs, refs_size, cand_size, level_size):
        self.bd, self.luma, self.rec, self.org, self.avail = bd, np.ascontiguousarray(luma), np.ascontiguousarray(rec), np.ascontiguousarray(org), np.ascontiguousarray(avail)
        self.pus, self.fill, self.runs = pus, fill, np.ascontiguousarray(np.asarray(runs, np.int32).reshape(-1, 3))
        self.refs_size, self.cand_size, self.level_size = int(refs_size), int(cand_size), int(level_size)

    def initial(self):
        """(refs, pred, rec, level) before the call"""
        return (np.full(self.refs_size, REFS_CANARY, np.int16), np.full(self.cand_size, PRED_CANARY, np.int16), np.full(self.cand_size, REC_CANARY, np.int16),
                np.full(self.level_size, LEVEL_CANARY, np.int32))

    def run_shapes(self):
        """the (w, h) of the run every PU lies in"""
        return np.repeat(self.runs[:, :2], np.maximum(self.runs[:, 2], 0), axis=0)

    def sub(self, keep):
        """the case of the PUs `keep` (indices in list order), runs rebuilt"""
        keep = np.asarray(keep)
        shapes = self.run_shapes()[keep]
        runs = []
        for s in shapes:
            if runs and runs[-1][0] == s[0] and runs[-1][1] == s[1]:
                runs[-1][2] += 1
            else:
                runs.append([int(s[0]), int(s[1]), 1])
        return Case(self.bd, self.luma, self.rec, self.org, self.avail, self.pus[keep].copy(), self.fill.reshape(-1, 2)[keep].reshape(-1).copy(), runs,
                    self.refs_size, self.cand_size, self.level_size)


def pu_ok(case, q, have_luma=True, gather=True):
    """the contract of include/vvcgpu.h for PU q"""
    u = case.pus[q]
    w, h = int(u["w"]), int(u["h"])
    rw, rh = (int(v) for v in case.run_shapes()[q])
    if not (rd.side_ok(w, 2) and rd.side_ok(h, 2) and w == rw and h == rh and u["cand_off"] % 4 == 0 and u["level_off"] % 4 == 0):
        return False
    if not all(-1 <= int(m) <= LM for m in u["mode"]) or (not have_luma and LM in [int(m) for m in u["mode"]]):
        return False
    if gather:
        T, L = ref_lengths(w, h)
        for c in range(2):
            f = case.fill[2 * q + c]
            if not (f["w"] == w and f["h"] == h and f["ref_off"] == u["ref_off"][c] and f["unit_w"] >= 1 and f["unit_h"] >= 1):
                return False
            if (T + int(f["unit_w"]) - 1) // int(f["unit_w"]) + (L + int(f["unit_h"]) - 1) // int(f["unit_h"]) + 1 > 192:
                return False
    return True


def at(buf, off):
    return C.c_void_p(buf.ctypes.data + buf.itemsize * int(off))


def gathered(case, q, c):
    """the packed references of component c of PU q (orc_intra_fill_refs over the fill descriptor)"""
    f = case.fill[2 * q + c]
    w, h = int(f["w"]), int(f["h"])
    out = np.zeros(sum(ref_lengths(w, h)) + 1, np.int16)
    rec = case.rec.reshape(-1)
    oracle().orc_intra_fill_refs(at(rec, f["rec_off"]), int(f["rec_stride"]), at(case.avail, f["flags_off"]), p(out), w, h, int(f["unit_w"]), int(f["unit_h"]), case.bd)
    return out


def predict(case, q, c, mode, refs, clp):
    u = case.pus[q]
    w, h = int(u["w"]), int(u["h"])
    pred = np.zeros((h, w), np.int16)
    if mode == LM:
        T = ref_lengths(w, h)[0]
        nb_above, nb_left = np.ascontiguousarray(refs[1:1 + w]), np.ascontiguousarray(refs[T + 1:T + 1 + h])
        oracle().orc_cclm_pred(at(case.luma.reshape(-1), u["luma_off"]), int(u["luma_stride"]), p(nb_above), p(nb_left), p(pred), w, w, h, int(u["above_avail"]),
                               int(u["left_avail"]), case.bd, case.bd, clp[0], clp[1])
    else:
        oracle().orc_intra_pred(p(refs), p(pred), w, w, h, mode, clp[0], clp[1])
    return pred


def restate(case, flags=0, clp=None, have_luma=True, gather=True, refs_given=None):
    """the entry over every PU -> dict(refs, pred, rec, level: the four buffers after the call; abs_sum uint32 [n][6][2]; dist uint64 [n][6][2]).
    gather False: the references are read from refs_given (the refs buffer stays as it is)"""
    clp = clp or (0, (1 << case.bd) - 1)
    n = len(case.pus)
    refs_b, pred_b, rec_b, level_b = case.initial()
    if not gather:
        refs_b = refs_given.copy()
    out = dict(refs=refs_b, pred=pred_b, rec=rec_b, level=level_b, abs_sum=np.full((n, SLOTS, 2), U32_MAX, np.uint32), dist=np.full((n, SLOTS, 2), U64_MAX, np.uint64))
    org_flat = case.org.reshape(-1)
    for q, u in enumerate(case.pus):
        if not pu_ok(case, q, have_luma, gather):
            continue
        w, h = int(u["w"]), int(u["h"])
        for c in range(2):
            ro = int(u["ref_off"][c])
            if gather:
                refs = gathered(case, q, c)
                refs_b[ro:ro + refs.size] = refs
            else:
                refs = np.ascontiguousarray(refs_b[ro:ro + sum(ref_lengths(w, h)) + 1])
            org = itc.block(org_flat, int(u["org_off"][c]), int(u["org_stride"]), w, h)
            for k in range(SLOTS):
                mode = int(u["mode"][k])
                if mode < 0:
                    continue
                pred = predict(case, q, c, mode, refs, clp)
                level, abs_sum, rec, dist = itc.code_block(org, pred, case.bd, 0, 0, int(u["qp"][c]), int(u["intra_slice"]), int(u["sign_hiding"]), clp)
                co, lo = int(u["cand_off"]) + (2 * k + c) * w * h, int(u["level_off"]) + (2 * k + c) * w * h
                if flags & WRITE_PRED:
                    pred_b[co:co + w * h] = pred.reshape(-1)
                rec_b[co:co + w * h] = rec.reshape(-1)
                level_b[lo:lo + w * h] = level.reshape(-1)
                out["abs_sum"][q, k, c], out["dist"][q, k, c] = abs_sum, dist
    return out


# ---- builders --------------------------------------------------------------------------------------------------------------------------------------
def place(rng, w, h):
    """a position on the unit grid with the block inside the plane and a row above and a column to the left of it (two for the luma block's columns)"""
    return UNIT * int(rng.integers(1, (CW - w) // UNIT + 1)), UNIT * int(rng.integers(1, (CH - h) // UNIT + 1))


def make(rng, bd, specs, pl=None):
    """specs: one dict per PU with w, h and any of modes (default cand_modes(34)), qp (a pair, or one value for both; default 32 + the bit-depth offset),
    intra, sbh, avail (see availability; default 'all'), pos.  The list is grouped by shape here (stable), every PU gets candidate regions of its own with
    canaries between."""
    luma, rec, org = pl if pl is not None else planes(rng, bd)
    order = sorted(range(len(specs)), key=lambda i: SHAPE_KEY(specs[i]))
    specs = [specs[i] for i in order]
    n = len(specs)
    pus, fill = np.zeros(n, abi.INTRA_CHROMA_PU), np.zeros(2 * n, abi.INTRA_FILL_DESC)
    avail, runs = [], []
    fo = ro = 0
    co, lo = 8, 4
    for q, s in enumerate(specs):
        w, h = s["w"], s["h"]
        x, y = s["pos"] if "pos" in s else place(rng, w, h)
        f = availability(w, h, x, y, s.get("avail", "all"), rng)
        T, L = ref_lengths(w, h)
        qp = s.get("qp", 32 + 6 * (bd - 8))
        qp = (qp, qp) if np.isscalar(qp) else qp
        a, l = cclm_flags(f, w, h)
        u = pus[q]
        for c in range(2):
            u["org_off"][c] = c * CW * CH + y * CW + x
            u["ref_off"][c] = ro
            fill[2 * q + c] = (c * CW * CH + y * CW + x, fo, ro, CW, w, h, UNIT, UNIT, 0, 0)
            ro += T + L + 1 + (q + c) % 3
        u["luma_off"], u["luma_stride"], u["org_stride"] = 2 * y * 2 * CW + 2 * x, 2 * CW, CW
        u["cand_off"], u["level_off"] = co, lo
        u["qp"], u["w"], u["h"], u["above_avail"], u["left_avail"] = qp, w, h, a, l
        u["intra_slice"], u["sign_hiding"], u["mode"] = s.get("intra", 1), s.get("sbh", 1), s.get("modes", cand_modes(34))
        avail.append(f)
        fo += f.size
        co += 2 * SLOTS * w * h + 4 * (1 + q % 3)
        lo += 2 * SLOTS * w * h + 4 * (1 + (q + 1) % 3)
        if runs and runs[-1][:2] == [w, h]:
            runs[-1][2] += 1
        else:
            runs.append([w, h, 1])
    return Case(bd, luma, rec, org, np.concatenate(avail), pus, fill, runs, ro + 8, co + 8, lo + 8)


def SHAPE_KEY(s):
    return (s["w"], s["h"])


def conditions(case, want):
    """the conditions the issue sets for a list, asserted by the generator and by the CPU test; -> the labels reached"""
    seen = set()
    shapes = set()
    for q, u in enumerate(case.pus):
        if not pu_ok(case, q):
            continue
        w, h = int(u["w"]), int(u["h"])
        shapes.add((w, h))
        modes = [int(m) for m in u["mode"]]
        for m, name in ((0, "planar"), (1, "DC"), (18, "HOR"), (50, "VER"), (LM, "LM")):
            if m in modes:
                seen.add(name)
        if 66 in modes[:4]:
            seen.add("VDIA substitution")
        dm = modes[5]
        if dm > 1 and dm not in (18, 50):
            pm = wide_angle(w, h, dm)
            if pm != dm and w != h:
                seen.add("wide-angle DM")
            elif 10 < pm < 58:
                seen.add("angular DM without PDPC")
        if LM in modes:
            seen.add("LM %d%d" % (int(u["above_avail"]), int(u["left_avail"])))
        if -1 in modes:
            seen.add("unused slot")
        f = case.fill[2 * q]
        if not case.avail[int(f["flags_off"]):int(f["flags_off"]) + n_units(w, h)].any():
            seen.add("no neighbour")
    served = want["abs_sum"] != U32_MAX
    for c in range(2):
        if (served[:, :, c] & (want["abs_sum"][:, :, c] == 0)).any():
            seen.add("abs_sum == 0, component %d" % c)
        if (served[:, :, c] & (want["abs_sum"][:, :, c] > 0)).any():
            seen.add("abs_sum > 0, component %d" % c)
    need = {"planar", "DC", "HOR", "VER", "LM", "VDIA substitution", "wide-angle DM", "angular DM without PDPC", "LM 00", "LM 01", "LM 10", "LM 11", "unused slot",
            "no neighbour", "abs_sum == 0, component 0", "abs_sum > 0, component 0", "abs_sum == 0, component 1", "abs_sum > 0, component 1"}
    assert need <= seen, sorted(need - seen)
    assert set(SHAPES) <= shapes, sorted(set(SHAPES) - shapes)
    return seen


def golden_specs(bd):
    """the list of the golden file: every shape of the issue, every mode class, LM under the four availability pairs, a PU with no neighbour, an unused
    slot, quantisers that leave levels and one that leaves none.  The large shapes carry few slots: the file stays small."""
    o = 6 * (bd - 8)
    mq = itc.max_qp(bd)
    return [dict(w=2, h=2, modes=cand_modes(50), qp=(22 + o, 27 + o)), dict(w=2, h=8, modes=cand_modes(61), qp=27 + o, avail=(1, 0)),
            dict(w=8, h=2, modes=cand_modes(5), qp=22 + o, avail=(0, 1), sbh=0), dict(w=4, h=4, modes=cand_modes(0), qp=(32 + o, 22 + o)),
            dict(w=4, h=4, modes=cand_modes(34), qp=27 + o, avail="none"), dict(w=8, h=8, modes=cand_modes(18), qp=27 + o, intra=0),
            dict(w=8, h=8, modes=cand_modes(26, lm=False), qp=22 + o, avail="random"), dict(w=8, h=8, modes=cand_modes(1), qp=mq, avail=(0, 0)),
            dict(w=4, h=16, modes=cand_modes(64), qp=(27 + o, 32 + o)), dict(w=16, h=16, modes=cand_modes(42), qp=22 + o, sbh=0),
            dict(w=16, h=16, modes=cand_modes(2), qp=32 + o, avail=(1, 0)), dict(w=32, h=8, modes=cand_modes(4), qp=27 + o, avail=(0, 1)),
            dict(w=32, h=32, modes=[0, -1, -1, -1, LM, 45], qp=(27 + o, 22 + o)), dict(w=64, h=64, modes=[-1, -1, -1, -1, LM, 30], qp=32 + o),
            dict(w=64, h=16, modes=[-1, 50, -1, -1, LM, 7], qp=27 + o, intra=0)]


def golden_case(g, bd):
    k = "bd%d_" % bd
    return Case(bd, g[k + "luma"], g[k + "rec"], g[k + "org"], g[k + "avail"], g[k + "pus"].view(abi.INTRA_CHROMA_PU).reshape(-1),
                g[k + "fill"].view(abi.INTRA_FILL_DESC).reshape(-1), g[k + "runs"], int(g[k + "refs_size"]), int(g[k + "cand_size"]), int(g[k + "level_size"])), int(g[k + "flags"])


def mixed_specs(rng, bd, n):
    """a random mixed list: every shape with both sides in 2..64 may occur (the small ones more often), random DMs, availability kinds, quantisers"""
    o = 6 * (bd - 8)
    small = [(w, h) for w in (2, 4, 8, 16) for h in (2, 4, 8, 16)]
    large = [(w, h) for w in (2, 4, 8, 16, 32, 64) for h in (2, 4, 8, 16, 32, 64) if max(w, h) >= 32]
    kinds = ["all", "random", (1, 0), (0, 1), "none", "all", (0, 0), "random"]
    specs = []
    for i in range(n):
        w, h = small[int(rng.integers(len(small)))] if i % 4 else large[(i // 4) % len(large)]
        dm = int(rng.integers(0, 67))
        modes = cand_modes(dm, lm=bool(i % 5))
        if i % 7 == 3:
            modes[int(rng.integers(0, 4))] = -1
        if max(w, h) >= 32:                                   # the large shapes keep a few slots: the restatement's time
            modes = [m if j in (i % 4, 4, 5) else -1 for j, m in enumerate(modes)]
        specs.append(dict(w=w, h=h, modes=modes, qp=(int(rng.integers(17, 38)) + o, int(rng.integers(17, 38)) + o), intra=int(rng.integers(0, 2)),
                          sbh=int(rng.integers(0, 2)), avail=kinds[i % len(kinds)]))
    return specs


def bound_case(bd):
    """a 64 x 64 PU whose original is the full-range checkerboard and whose LM reconstruction has the opposite phase: the luma reconstruction and the chroma
    neighbours carry the opposite checkerboard (one value per 2 x 2 luma samples), so the down-sampled luma is a checkerboard between a quarter and three
    quarters of the range and the fitted model (slope 2) maps it back onto the full range.  The residual lies in the band the 64-point transform zeroes
    out; at 10 bit the SSE is close to 64 x 64 x 1023^2 = 0.998 x 2^32, beyond a signed 32-bit sum.  Slot 0 is DC (a flat prediction: half of that).
    -> (case, restatement)"""
    mx = (1 << bd) - 1
    yy, xx = np.mgrid[0:CH, 0:CW]
    v = (((yy + xx) & 1) * mx).astype(np.int16)
    luma = np.repeat(np.repeat(v, 2, axis=0), 2, axis=1)
    rec, org = np.stack([v, v]), np.stack([mx - v, mx - v]).astype(np.int16)
    case = make(np.random.default_rng(1), bd, [dict(w=64, h=64, modes=[1, -1, -1, -1, LM, -1], qp=45 + 6 * (bd - 8), pos=(8, 6))], pl=(luma, rec, org))
    want = restate(case)
    assert (want["dist"][0, 4] > (1 << (2 * bd + 11))).all(), want["dist"][0]         # above half of 64 x 64 x (2^bd)^2: 2^31 at 10 bit
    return case, want
