"""Generates tests/golden/resi_rate.npz: level blocks whose CABAC rate is the COMPILED REFERENCE's, and runs of the compare of xEstimateInterResidualQT
whose costs are.  Build machine only (needs the reference tree and oracle/_ref/libvtmref.so, i.e. a build() where the reference exists):
    python tests/golden/gen_resi_rate.py

gen_resi_rate_driver.cpp -- compiled here against the reference's headers (the include set of oracle/Makefile's CXXFLAGS_REF, -fno-access-control) and
linked with libvtmref.so -- exposes the reference's own CABACWriter::residual_coding on a BitEstimator_Std (with resetBits / getEstFracBits around it),
the estimator's contexts as rows, the model tables through BinProbModel_Std's public interface, and RdCost::calcRdCost.  ref_choose() below is the loop
of InterSearch.cpp:4395-4568, written here from the reference's text over the driver's calcRdCost.  The tests' restatement (tests/resi_rate_cases.py) has
its own writing of both; the generator asserts that it reproduces every stored value.  Nothing of the reference is copied; only the data is stored.

Context snapshots: Ctx::init for two (qp, initId) pairs; the contexts after a run of mixed blocks; and two long runs of one block each, which drive
states to both ends of the state range (asserted below).  Every item carries its own row before and after its block."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

import resi_rate_cases as rrc  # noqa: E402
from oraclelib import p  # noqa: E402
from rd_pass_kit import save_golden  # noqa: E402
from vvcsoftware_vtm_amd.abi import INTER_RESI_SLOTS, INTER_RESI_TS, RESI_RATE_CTX_BYTES  # noqa: E402

REF = os.environ.get("REF", "/root/reference")


def driver():
    src = os.path.join(REF, "source", "Lib")
    inc = ["-I" + os.path.join(src, d) for d in ("", "CommonLib", "CommonLib/x86", "libmd5", "EncoderLib", "DecoderLib", "Utilities")]
    refdir = os.path.join(ROOT, "oracle", "_ref")
    out = os.path.join(tempfile.mkdtemp(), "librrref.so")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-fPIC", "-shared", "-msse4.1", "-w", "-DNDEBUG", "-fno-access-control"] + inc +
                          [os.path.join(HERE, "gen_resi_rate_driver.cpp"), "-o", out, "-L" + refdir, "-lvtmref", "-Wl,-rpath," + refdir])
    D = C.CDLL(out)
    D.rrref_code.restype = C.c_uint64
    D.rrref_cost.restype = C.c_double
    D.rrref_cost.argtypes = [C.c_double, C.c_uint64, C.c_uint64]
    return D


def ref_code(D, lv, it):
    """the reference's bits of one block from the estimator's current contexts, which move on"""
    lv = np.ascontiguousarray(lv, np.int32)
    assert it["emt_idx"] < 0 or it["emt_inter"] != it["emt_thr"]              # the reference ties both to CU::isIntra
    bits = D.rrref_code(p(lv), int(it["w"]), int(it["h"]), int(it["luma"]), int(it["dep_quant"]), int(it["sign_hiding"]), int(it["ts_flag"]),
                        int(it["emt_idx"]), int(it["emt_thr"]))
    assert bits != rrc.U64_MAX
    return bits


def row_of(D, luma):
    row = np.zeros(RESI_RATE_CTX_BYTES, np.uint8)
    D.rrref_row(int(luma), p(row))
    return row


# ---- the level patterns ------------------------------------------------------------------------------------------------------------------------
def patterns(rng, w, h, luma):
    """[(name, levels [w h], item fields)] of one shape: the smallest blocks at which each branch of residual_coding can go wrong"""
    scan, cg = rrc.scan_order(w, h)
    n, nsub = w * h, w * h // cg
    emt = luma and w <= 32 and h <= 32                                         # emt_tu_index: luma, up to EMT_INTRA / INTER_MAX_CU_WITH_QTBT; the host decides
    out = []

    def add(name, fill, **kw):
        a = np.zeros(n, np.int32)
        fill(a)
        out.append((name, a, kw))

    def at(a, pos, v):
        a[scan[pos]] = v

    add("dc", lambda a: at(a, 0, -3))
    add("last position", lambda a: at(a, n - 1, 5))                            # raster (w - 1, h - 1): the longest prefixes and suffixes of the shape
    add("dense small", lambda a: a.__setitem__(slice(None), np.where(rng.random(n) < 0.01, 1, rng.integers(-2, 3, n))))

    def rice(a):                                                               # small, medium and large magnitudes side by side, and the extremes
        m = min(n, 256)
        kind = rng.integers(0, 4, m)
        mag = np.where(kind == 0, rng.integers(0, 9, m), np.where(kind == 1, rng.integers(5, 31, m), np.where(kind == 2, rng.integers(17, 420, m), 0)))
        a[np.array(scan[:m])] = mag * rng.choice([-1, 1], m)
        at(a, 1, 32767)
        at(a, min(m - 1, 7), -32767)
        at(a, m - 1, 9)
    add("rice and escape", rice)
    add("sign hiding 3 apart", lambda a: (at(a, 0 if cg == 4 else 2, -1), at(a, 3 if cg == 4 else 5, 2)))
    if cg == 16:
        add("sign hiding 4 apart", lambda a: (at(a, 2, 1), at(a, 6, -4), at(a, 4, 1)))
    add("two levels", lambda a: (at(a, 1, 1), at(a, 3, -1)), emt_idx=0 if emt else -1, emt_thr=1)     # (the reference demands index 0 here)
    add("three levels", lambda a: (at(a, 0, 2), at(a, 1, 1), at(a, 3, -1)), emt_idx=1 if emt else -1, emt_thr=1)
    add("inter emt", lambda a: at(a, 2, 1), emt_idx=3 if emt else -1, emt_inter=1 if emt else 0)
    add("transform skip flag 0", lambda a: (at(a, 0, 6), at(a, 2, -1)), ts_flag=0)
    add("transform skip flag 1", lambda a: (at(a, 1, -2), at(a, min(n - 1, 9), 1)), ts_flag=1)
    add("all zero", lambda a: None)
    if nsub >= 4:
        def sparse(a):                                                         # empty groups between significant ones, under both group-flag contexts
            for sub in sorted(set([nsub - 1, nsub // 2, 1 + nsub // 3])):
                for k in rng.integers(0, cg, 3):
                    at(a, sub * cg + int(k), int(rng.integers(1, 4)) * int(rng.choice([-1, 1])))
        add("sparse groups", sparse)
        add("inferred significance", lambda a: (at(a, (nsub - 1) * cg + 1, 1), at(a, (nsub // 2) * cg, -2), at(a, cg, 7), at(a, 0, 1)))
    return out


def build_items(D, rng):
    """every pattern of every shape, channel type and flag pair from rotating snapshots -> arrays; D's slots 0..4 hold the snapshots"""
    level, items, before, after, bits, nsig, names = [], [], [], [], [], [], []
    trace, off, k = set(), 0, 0
    est, nxt = model(D)
    for luma in (1, 0):
        for (w, h) in rrc.SHAPES + ([] if luma else rrc.CHROMA_ONLY):
            for (dq, sbh) in rrc.FLAGS:
                for name, lv, kw in patterns(rng, w, h, luma):
                    it = rrc.make_item(off, len(items), w, h, luma, dq, sbh, **kw)
                    D.rrref_restore(k % 5)
                    k += 1
                    r0 = row_of(D, luma)
                    if lv.any():
                        b = ref_code(D, lv, it[0])
                        r1, ns = row_of(D, luma), int(np.count_nonzero(lv))
                    else:
                        b, r1, ns = 0, r0, 0                                   # the reference never codes an empty block: 0 and 0, the row as it was
                    want = rrc.restate_block(lv.reshape(h, w), it[0], r0, est, nxt, trace)
                    assert want[0] == b and want[1] == ns and np.array_equal(want[2], r1), (name, w, h, luma, dq, sbh, want[0], b)
                    level.append(lv); items.append(it); before.append(r0); after.append(r1); bits.append(b); nsig.append(ns)
                    names.append(name)
                    off += w * h
    # which branches the set reaches
    for need in [("group", 0, 0), ("group", 0, 1), ("group", 1, 0), ("group", 1, 1), ("inferred", "last"), ("inferred", "first"), ("hide", 3), ("hide", 4),
                 ("emt", 1, 2), ("emt", 1, 3), ("emt", 0, 1)] + [("rice", r, e) for r in range(3) for e in (False, True)]:
        assert need in trace, need
    return dict(level=np.concatenate(level), items=np.concatenate(items).view(np.uint8).reshape(-1, 32), ctx_before=np.array(before),
                ctx_after=np.array(after), bits=np.array(bits, np.uint64), num_sig=np.array(nsig, np.uint32))


def model(D):
    est, nxt = np.zeros(128, np.uint32), np.zeros(256, np.uint8)
    D.rrref_model(p(est), p(nxt))
    return est, nxt


def snapshots(D, rng):
    """fills the driver's slots: 0, 1 Ctx::init; 2 after a run of mixed blocks; 3, 4 after long runs of one block each"""
    D.rrref_init(32, 0); D.rrref_save(0)
    D.rrref_init(22, 2); D.rrref_save(1)
    D.rrref_init(27, 1)
    for i in range(40):
        luma = i & 1
        w, h = rrc.SHAPES[int(rng.integers(0, 7))]
        lv = rrc.random_block(rng, w, h)
        if lv.any():
            ref_code(D, lv, rrc.make_item(0, 0, w, h, luma, i % 3 == 0, i % 3 == 2)[0])
    D.rrref_save(2)
    big = np.full((16, 16), 9, np.int32)                                       # every flag 1, every time
    one = np.zeros((16, 16), np.int32); one[0, 0] = 1; one[15, 15] = -1         # every flag but two 0
    for slot, lv in ((3, big), (4, one)):
        D.rrref_init(37, 0)
        for i in range(120):
            for luma in (1, 0):
                ref_code(D, lv, rrc.make_item(0, 0, 16, 16, luma, 1, 0)[0])
        D.rrref_save(slot)
    rows = []
    for slot in range(5):
        D.rrref_restore(slot)
        rows += [row_of(D, 1), row_of(D, 0)]
    rows = np.array(rows)[:, :180]
    assert rows.min() <= 1 and rows.max() >= 124, (rows.min(), rows.max())      # both ends of the state range
    assert len(set(int(v) for v in rows.reshape(-1))) > 60


# ---- the compare ----------------------------------------------------------------------------------------------------------------------------------
def ref_choose(D, c):
    """:4395-4568 per item over the driver's calcRdCost; the Cb item of a Cr item first -> the outputs of the entry, and which branches were taken"""
    n, taken = len(c["tr"]), set()
    out = dict(slot=np.full(n, -1, np.int32), cbf=np.zeros(n, np.int32), abs_sum_out=np.full(n, rrc.U32_MAX, np.uint32),
               dist=np.full(n, rrc.U64_MAX, np.uint64), bits=np.full(n, rrc.U64_MAX, np.uint64), min_cost=np.full(n, rrc.DBL_MAX, np.float64))

    def component(i, prev_cbf):
        codes = [int(v) for v in c["tr"][i]]
        num = sum(1 for v in codes if v != -1)
        if codes[0] == -1 or codes[:num].count(-1) or any(v == INTER_RESI_TS for v in codes[:num - 1]) or int(c["zero_dist"][i]) == rrc.U64_MAX:
            return None
        check_ts = codes[num - 1] == INTER_RESI_TS
        weight = float(c["weight"][i])
        dist_part = lambda x: int(weight * float(int(x)))                      # getDistPart: (Distortion)(m_distortionWeight * distortion)
        min_cost, best = rrc.DBL_MAX, None
        for mode in range(num):
            abs_sum = int(c["abs_sum"][i][mode])
            if abs_sum == rrc.U32_MAX:
                if mode == 0:
                    return None
                continue                                                       # a slot the pixel pass did not serve: passed over
            first = mode == 0
            curr_bits, curr_dist, curr_cost, non_bits, non_dist, non_cost, cbf = 0, 0, 0.0, 0, 0, 0.0, int(abs_sum > 0)
            if first or abs_sum == 0:
                non_dist = dist_part(c["zero_dist"][i])
                non_bits = int(c["cbf_bits"][i][2 * prev_cbf])
                non_cost = D.rrref_cost(c["scale"], non_bits, non_dist)
            if abs_sum > 0:
                curr_bits = int(c["cbf_bits"][i][2 * prev_cbf + 1]) + int(c["frac_bits"][i][mode])
                curr_dist = dist_part(c["dist_resi"][i][mode])
                curr_cost = D.rrref_cost(c["scale"], curr_bits, curr_dist)
            elif mode == num - 1 and check_ts:
                curr_cost = rrc.DBL_MAX
            else:
                curr_bits, curr_dist, curr_cost, cbf = non_bits, non_dist, non_cost, 0
            if curr_cost < min_cost or (mode == num - 1 and check_ts and curr_cost == min_cost):
                if mode == num - 1 and check_ts and curr_cost == min_cost:
                    taken.add("tie")
                if first and (non_cost < curr_cost or abs_sum == 0):
                    taken.add("forced null" if abs_sum else "null")
                    cbf, abs_sum, curr_bits, curr_dist, curr_cost = 0, 0, non_bits, non_dist, non_cost
                min_cost, best = curr_cost, (mode, cbf, abs_sum, curr_dist, curr_bits, curr_cost)
        return best

    for i in range(n):
        prev_cbf = 0
        if c["prev"][i] != -1:
            cb = component(int(c["prev"][i]), 0) if 0 <= c["prev"][i] < n else None
            if cb is None:
                continue
            prev_cbf = cb[1]
            taken.add(("cr", prev_cbf))
        r = component(i, prev_cbf)
        if r is not None:
            out["slot"][i], out["cbf"][i], out["abs_sum_out"][i], out["dist"][i], out["bits"][i], out["min_cost"][i] = r
            if c["weight"][i] != 1.0 and float(c["weight"][i]) * float(int(c["zero_dist"][i])) != r[3] and r[1] == 0:
                taken.add("truncated")
    return out, taken


def build_choose(D):
    c = rrc.random_choose(4242, 160)
    n = len(c["tr"])
    # a transform-skip tie: slot 0 and the transform-skip slot at equal cost; a forced null; a Cr item behind a Cb item with and without a level
    c["tr"][0] = [0, INTER_RESI_TS, -1, -1, -1, -1]
    c["abs_sum"][0] = [5, 7] + [rrc.U32_MAX] * 4
    c["dist_resi"][0, :2] = 1000
    c["frac_bits"][0, :2] = 70000
    c["zero_dist"][0], c["prev"][0], c["weight"][0] = 900000, -1, 1.0
    c["tr"][1] = [0, -1, -1, -1, -1, -1]
    c["abs_sum"][1, 0], c["dist_resi"][1, 0], c["frac_bits"][1, 0], c["zero_dist"][1], c["prev"][1] = 3, 5000, 1 << 21, 5001, -1
    for i, cb_abs in ((2, 4), (4, 0)):
        c["tr"][i] = c["tr"][i + 1] = [0, -1, -1, -1, -1, -1]
        c["abs_sum"][i, 0], c["abs_sum"][i + 1, 0] = cb_abs, 6
        c["dist_resi"][i, 0], c["frac_bits"][i, 0], c["zero_dist"][i] = 100, 40000, 1 << 19
        c["dist_resi"][i + 1, 0], c["frac_bits"][i + 1, 0], c["zero_dist"][i + 1] = 300, 50000, 1 << 18
        c["prev"][i], c["prev"][i + 1] = -1, i
        c["weight"][i] = c["weight"][i + 1] = 1.37
    assert n > 8
    out, taken = ref_choose(D, c)
    for need in ("tie", "forced null", "null", ("cr", 0), ("cr", 1), "truncated"):
        assert need in taken, (need, taken)
    assert out["slot"][0] == 1 and (out["slot"] == -1).any() and len(set(out["slot"])) >= 5
    want = rrc.choose(c["tr"], c["abs_sum"], c["dist_resi"], c["zero_dist"], c["frac_bits"], c["cbf_bits"], c["prev"], c["weight"], c["scale"])
    for key in out:
        assert want[key].tobytes() == out[key].tobytes(), key
    g = {"choose_" + k: v for k, v in c.items() if k not in ("weight", "scale")}
    g["choose_weight"] = c["weight"].view(np.uint64)
    g["choose_scale"] = np.array([c["scale"]], np.float64).view(np.uint64)
    g.update({"choose_out_" + k: (v.view(np.uint64) if v.dtype == np.float64 else v) for k, v in out.items()})
    return g


def main():
    D = driver()
    rng = np.random.default_rng(9100)
    snapshots(D, rng)
    est, nxt = model(D)
    g = dict(est_bits=est, next_state=nxt)
    g.update(build_items(D, rng))
    g.update(build_choose(D))
    print("%d blocks, %d levels, %d runs of the compare" % (len(g["bits"]), g["level"].size, len(g["choose_tr"])))
    save_golden(os.path.join(HERE, "resi_rate.npz"), g)


if __name__ == "__main__":
    main()
