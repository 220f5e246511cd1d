"""Descriptor lists for the tests of the two stand-alone rate-distortion quantisers, vvcgpu_rdoq_batch and vvcgpu_depquant_batch, with what the oracle
(orc_rdoq / orc_depquant, each pinned to the compiled reference by tests/test_oracle_golden.py) makes of them.  For the RDOQ lists the oracle's branch
counters (orc_rdoq_events) are kept per TU, so that tests/test_rdoq_cases_cpu.py can prove what the inputs reach before the device sees them.
Layout of every list: coefficient and level blocks at multiples of 16 with gaps of 16 * (i mod 3) elements between them, the gaps filled with canaries
(levels: compared with the device's buffer; coefficients: large values that a read past a block would pick up); the second half of a list has its level
blocks 32 elements further on than its coefficient blocks, so the two offsets differ.  The rate tables come from all rows of tests/golden/rdoq.npz and
tests/golden/depquant.npz (any table is a valid input for any shape).
numpy only: the CPU tests load this file without torch."""
import ctypes as C
import functools
import os

import numpy as np

from oraclelib import oracle, p
from vvcsoftware_vtm_amd import abi

HERE = os.path.dirname(os.path.abspath(__file__))
SIDES = (4, 8, 16, 32, 64)
LEVEL_CANARY = 0x5A5A5A5A
COEF_CANARY = 32767                                                          # a full-scale coefficient where none belongs
RDOQ, DEPQUANT = "rdoq", "depquant"
DESC = {RDOQ: abi.RDOQ_DESC, DEPQUANT: abi.DEPQUANT_DESC}
RATES = {RDOQ: abi.RDOQ_RATES, DEPQUANT: abi.DQ_RATES}

# orc_rdoq_events, in the order of oracle/restate/rdoq.cpp's RdoqEvent
EVENTS = ("level_capped", "cg_empty", "cg_nnz_before_pos0_zero", "cg_zeroed", "last_kept", "last_truncated", "last_zero", "last_walk_ended_gt1",
          "sbh_new", "sbh_new_before_first", "sbh_up", "sbh_down", "sbh_down_to_zero", "sbh_bonus_chosen", "sbh_forced_at_cap", "sbh_refused_by_sign",
          "escape_rice0", "escape_rice1", "escape_rice2", "rice0", "rice1", "rice2")
EV = {name: i for i, name in enumerate(EVENTS)}


def all_shapes():
    return [(w, h) for w in SIDES for h in SIDES]


def max_qp(bd):
    """the largest QpParam::Qp of a component: 63 plus the bit-depth offset"""
    return 63 + 6 * (bd - 8)


def rates_of(kind):
    g = np.load(os.path.join(HERE, "golden", kind + ".npz"))
    return np.ascontiguousarray(g["rates"]).view(RATES[kind]).reshape(-1)


def read_events():
    """the counters of this thread's orc_rdoq calls since the last read (the read clears them)"""
    out = np.zeros(len(EVENTS), np.uint32)
    oracle().orc_rdoq_events(p(out))
    return out


class Case:
    """descs: the descriptor array; coef: the coefficient buffer; total: total_coeffs of the call; want_level / want_sum: the level buffer (canaries in the
    gaps) and abs_sum the oracle gives; events [n][len(EVENTS)]: the oracle's counters per TU (RDOQ only)"""
    def __init__(self, kind, bd, descs, coef, rates, level_size, total):
        self.kind, self.bd, self.descs, self.coef, self.rates, self.level_size, self.total = kind, bd, descs, coef, rates, level_size, total
        n = len(descs)
        self.want_level = np.full(level_size, LEVEL_CANARY, np.int32)
        self.want_sum = np.zeros(n, np.uint32)
        self.events = np.zeros((n, len(EVENTS)), np.int64)
        o = oracle()
        o.orc_rdoq.restype = o.orc_depquant.restype = C.c_uint32
        read_events()
        for i, d in enumerate(descs):
            w, h, co, lo = int(d["w"]), int(d["h"]), int(d["coeff_off"]), int(d["level_off"])
            src = np.ascontiguousarray(coef[co:co + w * h])
            lv = np.zeros(w * h, np.int32)
            row = C.c_void_p(rates.ctypes.data + int(d["rates_idx"]) * rates.itemsize)
            if kind == RDOQ:
                self.want_sum[i] = o.orc_rdoq(p(src), p(lv), w, h, int(d["luma"]), bd, int(d["qp"]), C.c_double(float(d["lambda"])), int(d["sign_hiding"]), row)
                self.events[i] = read_events()
            else:
                self.want_sum[i] = o.orc_depquant(p(src), p(lv), w, h, int(d["luma"]), bd, int(d["qp"]), C.c_double(float(d["lambda"])), row)
            self.want_level[lo:lo + w * h] = lv

    def tu_level(self, i):
        d = self.descs[i]
        return self.want_level[int(d["level_off"]):int(d["level_off"]) + int(d["w"]) * int(d["h"])]

    def cell_events(self, w, h):
        sel = (self.descs["w"] == w) & (self.descs["h"] == h)
        return self.events[sel].sum(0)


def make(kind, bd, specs, rates=None, offsets=None, total=None):
    """specs: dicts of w, h, coef [w * h] int32, qp, lam, luma, sbh, rates_idx -> Case.  offsets: the coefficient offset of every block where the caller
    chooses them (multiples of 16); total: total_coeffs where the caller wants more than the list's own extent"""
    rates = rates_of(kind) if rates is None else rates
    n = len(specs)
    descs = np.zeros(n, DESC[kind])
    co = 0
    for i, s in enumerate(specs):
        if offsets is not None:
            co = offsets[i]
        assert co % 16 == 0
        sz = s["w"] * s["h"]
        descs[i]["coeff_off"], descs[i]["level_off"] = co, co + (32 if i >= (n + 1) // 2 else 0)
        descs[i]["lambda"], descs[i]["qp"], descs[i]["rates_idx"] = s["lam"], s["qp"], s["rates_idx"] % len(rates)
        descs[i]["w"], descs[i]["h"], descs[i]["luma"] = s["w"], s["h"], s["luma"]
        if kind == RDOQ:
            descs[i]["sign_hiding"] = s["sbh"]
        co += sz + 16 * (i % 3)
    ends = descs["coeff_off"] + descs["w"].astype(np.int64) * descs["h"]
    extent = int(ends.max())
    order = np.argsort(descs["coeff_off"])
    assert (descs["coeff_off"][order][1:] >= ends[order][:-1]).all()                     # blocks are disjoint
    total = extent if total is None else total
    assert total >= extent and total % 16 == 0
    coef = np.full(total, COEF_CANARY, np.int32)
    for d, s in zip(descs, specs):
        coef[int(d["coeff_off"]):int(d["coeff_off"]) + s["w"] * s["h"]] = s["coef"]
    return Case(kind, bd, descs, coef, rates, extent + 32 + 16, total)


# ---- the input families ----------------------------------------------------------------------------------------------------------------------------
def q_step(w, h, qp, bd):
    """the coefficient magnitude of one quantiser step: 2^((qp - 4) / 6) (g_quantScales[0] = 2^14 / 0.625) times 2^transformShift"""
    return 2.0 ** ((qp - 4) / 6.0) * 2.0 ** (15 - bd - np.log2(w * h) / 2)


def qp_lambda(qp):
    """the encoder's order of magnitude for a QP: 0.57 * 2^((qp - 12) / 3) of the QP with its bit-depth offset (the encoder scales lambda by that offset
    too: the distortion of an RDOQ cost is in the units of the bit depth)"""
    return 0.57 * 2.0 ** ((qp - 12) / 3.0)


def clip16(c):
    return np.clip(c, -32768, 32767).astype(np.int32).reshape(-1)


def fam_sparse(rng, w, h, bd, j, qp=None):
    """about two steps at DC with an exponential decay, plus isolated spikes of 0.4 .. 1.6 steps on 4 % or 30 % of the positions; lambda of the QP x {1, 4,
    16} (variant j walks the combinations): groups without a level, groups the cost test zeroes, lone levels at position 0, a last position that moves,
    every sign-hiding outcome at levels of 0 .. 2 (the denser spikes put several levels of one into the last group)"""
    qp = int(rng.integers(22, 38)) + 6 * (bd - 8) if qp is None else qp
    step = q_step(w, h, qp, bd)
    yy, xx = np.mgrid[0:h, 0:w]
    c = rng.normal(0, 1, (h, w)) * step * 2.2 * np.exp(-(xx / w * 3 + yy / h * 3))
    c += (rng.random((h, w)) < (0.04, 0.3)[j % 2]) * rng.choice([-1, 1], (h, w)) * step * rng.uniform(0.4, 1.6, (h, w))
    return clip16(c), qp, qp_lambda(qp) * (1, 4, 16)[j // 2 % 3]


def fam_dense(rng, w, h, bd, j, qp=None):
    """every coefficient N(0, 1) x step x {1, 3, 12, 40, 120}; lambda of the QP x {0.25, 1}: Rice parameters 1 and 2 and the escape codes; at one step, new
    levels in front of a group's first one; at 120 steps, levels beyond 255 (the trellis keeps its level histories in bytes)"""
    qp = int(rng.integers(10, 30)) + 6 * (bd - 8) if qp is None else qp
    step = q_step(w, h, qp, bd)
    c = rng.normal(0, 1, (h, w)) * step * (40, 120, 12, 3, 1)[j % 5]
    return clip16(c), qp, qp_lambda(qp) * (0.25, 1)[j % 2]


def fam_cap(rng, w, h, bd):
    """full-scale coefficients at QP 0 .. 2: levels beyond 32767 where the shape's scaling allows them"""
    return rng.choice(np.array([32767, -32768, 32000, -32001], np.int32), w * h), int(rng.integers(0, 3)), 0.7


def spec(w, h, coef, qp, lam, luma, sbh, rates_idx):
    return dict(w=w, h=h, coef=coef, qp=qp, lam=lam, luma=luma, sbh=sbh, rates_idx=rates_idx)


# ---- the cases -------------------------------------------------------------------------------------------------------------------------------------
PER_SHAPE = 12
# what shapes_case wants every shape to reach (the group events only where a TU has four or more groups); tests/test_rdoq_cases_cpu.py states its own list
SHAPE_EVENTS = ("sbh_new", "sbh_new_before_first", "sbh_up", "sbh_down", "sbh_down_to_zero", "sbh_bonus_chosen", "sbh_refused_by_sign",
                "escape_rice0", "escape_rice1", "escape_rice2", "rice0", "rice1", "rice2", "last_walk_ended_gt1")
GROUP_EVENTS = ("cg_empty", "cg_zeroed", "cg_nnz_before_pos0_zero", "last_truncated", "last_kept", "last_zero")


def candidates(bd, w, h):
    """the seeded pool of one shape: sparse and dense TUs in turn; candidate 0 runs at QP 0 and candidate 1 at the largest QP; sign hiding is off for every
    fourth, luma and chroma alternate in pairs.  Small shapes get a larger pool: a 4x4 TU decides sixteen coefficients, a 64x64 TU 4096"""
    rng = np.random.default_rng(4100 + bd * 10000 + w * 100 + h)
    out = []
    for j in range(max(48, min(768, 98304 // (w * h)))):
        qp = 0 if j == 0 else max_qp(bd) if j == 1 else None
        coef, qp, lam = (fam_sparse, fam_dense)[j % 2](rng, w, h, bd, j // 2, qp)
        out.append(spec(w, h, coef, qp, lam, (j >> 1) & 1, int(j % 4 != 3), int(rng.integers(0, 1 << 16))))
    return out


@functools.lru_cache(maxsize=None)
def shapes_specs(bd):
    """per shape the first four candidates, then for every wanted event that these do not reach the first candidate of the pool that does (found with the
    oracle's counters: a choice of seeds), then the next candidates up to PER_SHAPE; all shapes shuffled"""
    specs = []
    for (w, h) in all_shapes():
        pool = candidates(bd, w, h)
        ev = make(RDOQ, bd, pool).events
        take = [0, 1, 2, 3]
        for name in SHAPE_EVENTS + (GROUP_EVENTS if w * h >= 64 else ()):
            if not ev[take, EV[name]].any():
                hit = np.flatnonzero(ev[:, EV[name]])
                if len(hit):
                    take.append(int(hit[0]))
        take += [j for j in range(len(pool)) if j not in take][:max(0, PER_SHAPE - len(take))]
        specs += [pool[j] for j in sorted(take)]
    order = np.random.default_rng(4100 + bd).permutation(len(specs))     # the teams of a wavefront hold different shapes
    return tuple(specs[i] for i in order)


def shapes_case(bd, kind=RDOQ):
    """every shape, at least PER_SHAPE TUs of each from the sparse and the dense family, in a fixed random order (the trellis gets the same coefficients)"""
    case = make(kind, bd, shapes_specs(bd))
    shape_id = case.descs["w"].astype(np.int32) * 256 + case.descs["h"]
    quads = shape_id[:len(shape_id) // 4 * 4].reshape(-1, 4)
    assert (np.array([len(set(q)) for q in quads]) >= 3).mean() > 0.8    # most wavefronts of the RDOQ kernel (four teams) mix shapes
    return case


CAP_SHAPES = [(w, h) for (w, h) in all_shapes() if w * h >= 512]
CAP_PER_SHAPE = 6


def cap_case():
    """bit depth 10, the ten shapes with at least 512 coefficients, full-scale input at QP 0 .. 2 with sign hiding on: capped levels, and groups whose
    cheapest parity fix would raise a level of 32767"""
    rng = np.random.default_rng(4300)
    specs = []
    for (w, h) in CAP_SHAPES:
        for j in range(CAP_PER_SHAPE):
            coef, qp, lam = fam_cap(rng, w, h, 10)
            specs.append(spec(w, h, coef, qp, lam, j % 2, 1, int(rng.integers(0, 1 << 16))))
    order = np.random.default_rng(4301).permutation(len(specs))
    return make(RDOQ, 10, [specs[i] for i in order])


def margin_case(bd):
    """per shape one sparse TU at the two neighbouring doubles of lambda between which the oracle's decision for the whole block turns from coded to all
    zero (found by bisection on the oracle alone): the comparison `total < bestCost` of the last-position walk decided by the last bit of two cost chains,
    one of which holds the uncoded cost of every position behind the last level"""
    rng = np.random.default_rng(4400 + bd)
    o = oracle()
    o.orc_rdoq.restype = C.c_uint32
    rates = rates_of(RDOQ)
    specs = []
    for k, (w, h) in enumerate(all_shapes()):
        luma, ri = k % 2, int(rng.integers(0, len(rates)))
        row = C.c_void_p(rates.ctypes.data + ri * rates.itemsize)
        lv = np.zeros(w * h, np.int32)
        while True:
            coef, qp, lam = fam_sparse(rng, w, h, bd, 0)
            coded = lambda x: o.orc_rdoq(p(coef), p(lv), w, h, luma, bd, qp, C.c_double(x), 1, row) > 0
            lo, hi = lam, lam * 4096
            if coded(lo) and not coded(hi):
                break
        while np.nextafter(lo, hi) < hi:
            mid = lo + (hi - lo) / 2
            lo, hi = (mid, hi) if coded(mid) else (lo, mid)
        specs += [spec(w, h, coef, qp, lo, luma, 1, ri), spec(w, h, coef, qp, hi, luma, 1, ri)]
    read_events()
    case = make(RDOQ, bd, specs)
    assert (case.want_sum[0::2] > 0).all() and (case.want_sum[1::2] == 0).all()
    return case


PACKING_COUNTS = (1, 3, 4, 5, 15, 16, 17, 63, 64, 65)
PACKING_SHAPES = ((64, 64), (4, 4), (8, 4), (16, 16), (4, 4), (4, 4), (32, 8))


def packing_zero_slots(n):
    """-> {team slot: TU index} of the all-zero TUs of packing_case(n): one per slot of the four-team wavefront, each in a wavefront of its own, spread over
    the batch; TU 0 stays live, so a batch of one TU is a live one"""
    stride = max(1, n // 16)
    out = {}
    for j in range(4):
        i = 4 * j * stride + (j + 1) % 4
        if i < n:
            out[(j + 1) % 4] = i
    return out


def packing_case(n, kind=RDOQ, bd=10):
    """n TUs whose shapes cycle through PACKING_SHAPES (a period of 7 against wavefronts of 4 or 16 TUs: a 64x64 TU sits beside 4x4 TUs, in every slot over
    the batch), with an all-zero TU in each team slot (i mod 4) where n allows it"""
    rng = np.random.default_rng(4500 + n)
    zero = set(packing_zero_slots(n).values())
    specs = []
    for i in range(n):
        w, h = PACKING_SHAPES[i % len(PACKING_SHAPES)]
        coef, qp, lam = (fam_sparse, fam_dense)[i % 2](rng, w, h, bd, i // 2)
        if i in zero:
            coef = np.zeros(w * h, np.int32)
        specs.append(spec(w, h, coef, qp, lam, i % 3 != 0, int(i % 5 != 4), int(rng.integers(0, 1 << 16))))
    return make(kind, bd, specs)


WORKSPACE_SHAPES = ([(64, 64), (64, 16), (16, 64)], [(16, 16), (32, 64), (8, 32), (4, 4)])


def workspace_cases(kind=RDOQ, bd=10):
    """two lists for one workspace: blocks of the second start where blocks of the first start, with other shapes (its 32x64 block covers the first list's
    64x16 and 16x64 blocks), and both calls name the same total_coeffs, so every workspace array lies where it lay"""
    rng = np.random.default_rng(4700)
    first = []
    for k, (w, h) in enumerate(WORKSPACE_SHAPES[0]):
        coef, qp, lam = (fam_dense, fam_sparse)[k % 2](rng, w, h, bd, k)
        first.append(spec(w, h, coef, qp, lam, 1, 1, 7 + k))
    c1 = make(kind, bd, first)
    o1 = [int(o) for o in c1.descs["coeff_off"]]
    offs = [o1[0], o1[1], o1[0] + 512, o1[1] + 32 * 64 + 16]              # 16x16 and 8x32 inside the 64x64 block's extent, 32x64 over the two others
    second = []
    for k, (w, h) in enumerate(WORKSPACE_SHAPES[1]):
        coef, qp, lam = (fam_sparse, fam_dense)[k % 2](rng, w, h, bd, k)
        second.append(spec(w, h, coef, qp, lam, k % 2, 1, 40 + k))
    c2 = make(kind, bd, second, offsets=offs)
    total = max(c1.total, c2.total)
    return make(kind, bd, first, total=total), make(kind, bd, second, offsets=offs, total=total)
