"""The threading contract of include/vvcgpu.h -- re-entrant entry points, one stream per host thread -- run for real: several host threads, each on
its own stream, call different entry points at the same time and compare every result bit for bit with the oracle.

The job table (`job_table`, no GPU needed) holds small calls that between them touch every kind of state csrc/lib.hip shares between threads:
the slot table, the per-stream scratch (growing inside a call and between calls), the identity array, the two alternating counter sets, the
per-device table images and the thread-local error text.  The expectations come from oraclelib.oracle(), computed once, serially, in the main thread
(liboracle.so makes no promise about threads, and the expectation must not come from the code under test).

What a defect in each kind of shared state would look like (argued, not provoked: a deliberately broken library may fault the device).  Thread t starts
its pass at job t, so jobs at table positions a and b run at the same time on threads whose indices differ by b - a:
- slot table (a vector that re-allocates under push_back and shrinks under vvcgpu_stream_release): any call beside a thread's first call on a new stream
  or its release, e.g. `mc_batch` beside `me_batch 64 PUs`.  A lookup that lands in another stream's slot hands out that stream's scratch: the work list of
  mc_batch is overwritten by the other call's claims -> PUs of `dst` keep their initial -5 or hold another PU's samples.
- scratch: `me_batch 6000 PUs` (outgrows the buffer inside the call) or `resi_chain_batch` (the 100 MB claim) beside `quant_batch` / `sad_search`.  A buffer
  shared between streams, or an outgrown one freed before its queued readers ran: SEARCH_BEST / FRAC_RESULT records of some PUs wrong, large TUs of
  quant_batch left at the initial 9 with wrong abs sums.
- identity array: `resi_chain_runs_batch 256x128` beside `resi_chain_runs_batch 512x320` (two positions apart).  Shared between streams, the larger call
  would retire the array under the smaller call's queued kernels (the event guards one stream only); lost, the class lists are garbage: TUs skipped
  (`level` keeps 0x5A5A5A5A, `rec` keeps the prediction) or served twice, abs sums wrong.
- counter sets: `dist_batch` beside `mc_batch` / `resi_chain_batch`, and `tr_fwd_batch` + `dequant_tr_inv_batch` (two sets in a row).  One set handed to two
  streams, or the alternation lost: list lengths counted by two kernels at once or starting above zero -> 128x128 blocks of dist_batch keep the POISON
  bytes or a wrong sum, classes of PUs / TUs missing from `dst` / `level`, de-quantised coefficients of whole classes left at the initial 3.
- table images: `mc_batch .. 8 bit` beside `mc_batch .. 10 bit` (two keys), `frac_refine`, the transform jobs; from a cold library the threads' first
  calls race to build them.  An image used before it is complete, or the wrong key's: every sample of the 16x16 luma / 8x8 chroma PUs of mc_batch, the
  costs of frac_refine, the coefficients of tr_fwd_batch differ from the oracle's.
- error text: the refused `tr_fwd_batch` (bit depth 7) beside every other call.  Were the text process-wide, another thread would read "bit depth 7"
  from vvcgpu_last_error() at its end, or the refusing thread's VvcGpuError would carry another call's text."""
import ctypes as C
import os
import threading
import time

import numpy as np
import pytest
import torch

import cases
from oraclelib import oracle, p

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
POISON = 0xA5                  # byte pattern of an output tensor the binding allocates itself, written behind every use (see collect)


class Job:
    """name; inputs {name: numpy array} (every thread uploads its own copy); expected [numpy array]; initial [numpy array | None], one per expected
    output: the contents of the output buffer in front of every call (None: vvcsoftware_vtm_amd.ops allocates that output itself);
    launch(dev, outs) -> [device tensor] makes the library calls on the current stream (dev: the inputs on the device, outs: fresh device copies
    of `initial`); calls: the entry points `launch` goes through (for the messages and the call count)."""

    def __init__(self, name, inputs, expected, initial, launch, calls):
        assert len(expected) == len(initial)
        self.name, self.inputs, self.expected, self.initial, self.launch, self.calls = name, inputs, expected, initial, launch, calls

    def upload(self):
        """-> (inputs on the device, initial output contents on the device), allocated on the current stream"""
        dev = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in self.inputs.items()}
        init = [None if a is None else torch.from_numpy(_plain(a)).cuda() for a in self.initial]
        return dev, init

    def fresh(self, init):
        return [None if t is None else t.clone() for t in init]

    def collect(self, tensors):
        """waits for the CURRENT stream only, copies the outputs to the host; an output the binding allocated itself is then overwritten with POISON
        bytes, so that the allocator's next block for it cannot already hold the right answer of the previous round"""
        torch.cuda.current_stream().synchronize()
        got = [t.cpu().numpy() for t in tensors]
        for t, a in zip(tensors, self.initial):
            if a is None:
                t.view(torch.uint8).fill_(POISON)
        return got

    def run(self, dev, init):
        return self.collect(self.launch(dev, self.fresh(init)))

    def mismatches(self, got):
        """[] when every output equals the expectation bit for bit, else one text per differing output"""
        bad = []
        for i, (g, e) in enumerate(zip(got, self.expected)):
            g8, e8 = _plain(g).view(np.uint8).reshape(-1), _plain(e).view(np.uint8).reshape(-1)
            if g8.size != e8.size:
                bad.append("output %d: %d bytes, expected %d" % (i, g8.size, e8.size))
            elif not np.array_equal(g8, e8):
                item = _plain(e).dtype.itemsize
                ndiff = int(np.any((g8 != e8).reshape(-1, item), axis=1).sum())
                bad.append("output %d: %d of %d elements differ" % (i, ndiff, e8.size // item))
        return bad


def _plain(a):
    """a structured or plain array as a contiguous array torch can take (structured records as bytes)"""
    a = np.ascontiguousarray(a)
    if a.dtype.fields is not None:
        return a.view(np.uint8).reshape(a.shape + (a.dtype.itemsize,))
    if a.dtype in (np.uint16, np.uint32, np.uint64):
        return a.view({2: np.int16, 4: np.int32, 8: np.int64}[a.dtype.itemsize])
    return a


def _ops():
    from vvcsoftware_vtm_amd import ops
    return ops


def _desc_dev(dev, key):
    return dev[key].view(torch.uint8).reshape(-1)


# ---- the jobs ---------------------------------------------------------------------------------------------------------------
def _mc_job(bd, bi):
    """vvcgpu_mc_batch: per-stream work lists + a counter set; the matrix-core table image of bit depth `bd` (16x16 luma / 8x8 chroma PUs)"""
    ops = _ops()
    rng = np.random.default_rng(100 + 2 * bd + bi)
    mx, W, H, M = (1 << bd) - 1, 320, 192, 8
    r0, r1 = cases.rand_plane(rng, H, W, bd, "smooth"), cases.rand_plane(rng, H, W, bd, "smooth")
    shapes = [(16, 16, 1)] * 160 + [(8, 8, 0)] * 81 + [(4, 4, 1), (8, 4, 0), (32, 8, 1), (64, 64, 1), (12, 16, 1), (2, 2, 0), (128, 128, 1), (24, 24, 0)] * 3
    rows, doff = [], 0
    for (w, h, luma) in shapes:
        nf = 16 if luma else 32
        x0, y0, x1, y1 = (int(rng.integers(M, W - w - M)), int(rng.integers(M, H - h - M)), int(rng.integers(M, W - w - M)), int(rng.integers(M, H - h - M)))
        fx, fy, fx1, fy1 = [int(v) for v in rng.integers(0, nf, 4)]
        rows.append((y0 * W + x0, y1 * W + x1, doff, W, W, w, w, h, fx, fy, fx1, fy1, luma, bi, 0))
        doff += w * h
    d = np.array(rows, dtype=ops.MC_DESC)
    init = np.full(doff, -5, np.int16)
    want = init.copy()
    oracle().orc_mc_batch(p(r0), p(r1), p(want), p(d), len(d), bd, 0, mx)

    def launch(dev, outs):
        ops.mc_batch(dev["r0"], dev["r1"], outs[0], _desc_dev(dev, "d"), len(d), bd, (0, mx))
        return outs
    return Job("mc_batch %s %d bit" % ("bi" if bi else "uni", bd), {"r0": r0, "r1": r1, "d": _plain(d)}, [want], [init], launch, ["vvcgpu_mc_batch"])


_ME = {}


def _me_job(n):
    """vvcgpu_me_batch, the call of tests/test_gpu_edges.py::test_me_batch_scratch_grows_inside_the_chain: the TZ search's and the refinement's workspace
    from ONE scratch scope; with n = 6000 on a young stream a later claim outgrows the buffer while the earlier claims stay in use"""
    ops = _ops()
    W, H, M, bd, w, h = 512, 320, 160, 10, 16, 16
    if not _ME:
        rng = np.random.default_rng(77)
        _ME["org"], _ME["ref"] = cases.tz_planes(rng, W, H, M, bd, motion=(3, 2))
        _ME["lists"] = {k: cases.tz_pus(rng, k, W, H, M, [(w, h)], flags_choices=(0, 1), spread=8) for k in (64, 6000)}
    org, ref_, pus = _ME["org"], _ME["ref"], _ME["lists"][n]
    cfg = cases.tz_cfg(W, H, M, 9.5, search_range=32)
    O = oracle()
    wb = np.zeros(n, cases.BEST)
    O.orc_tz_search(p(org), W, p(ref_), ref_.shape[1], p(pus), n, p(cfg), p(wb))
    blk = np.zeros(n, ops.FRAC_BLK)
    blk["org_x"], blk["org_y"] = pus["org_x"], pus["org_y"]
    blk["ref_x"], blk["ref_y"] = pus["ref_x"] + wb["x"], pus["ref_y"] + wb["y"]
    blk["mv_x"], blk["mv_y"] = wb["x"], wb["y"]
    wf = np.zeros(n, ops.FRAC_RESULT)
    for i in range(n):                                                     # every PU has its own predictor
        m = ops.MvCost(9.5, int(pus["pred_hor"][i]), int(pus["pred_ver"][i]), 0, 0)
        O.orc_frac_refine(p(org), W, p(ref_), ref_.shape[1], p(blk[i:i + 1]), 1, w, h, bd, 0, (1 << bd) - 1, 1, C.byref(m), p(wf[i:i + 1]))

    def launch(dev, outs):
        return list(ops.me_batch(dev["org"], dev["ref"], _desc_dev(dev, "pus"), n, w, h, cfg, bd, use_hadamard=True))
    return Job("me_batch %d PUs" % n, {"org": org, "ref": ref_, "pus": _plain(pus)}, [wb, wf], [None, None], launch, ["vvcgpu_me_batch"])


def _rc_descs(tus, W, coffs):
    ops = _ops()
    d = np.zeros(len(tus), ops.RC_DESC)
    for i, (x, y, w, h, th, tv, qp, intra, sbh) in enumerate(tus):
        d[i] = (y * W + x, y * W + x, y * W + x, coffs[i], W, W, W, w, h, th, tv, intra, sbh, qp, (0, 0))
    return d


def _resi_chain_job(W, H):
    """vvcgpu_resi_chain_batch: class lists in scratch (with the 100 MB fall-back area: the largest claim of the table, it retires a young stream's
    buffer), a counter set as the list header, the transform tables and the f16 image.  Two sizes."""
    from test_gpu_resichain import oracle_chain, tile
    ops = _ops()
    rng = np.random.default_rng(W + H)
    bd, mx = 10, 1023
    org = cases.rand_plane(rng, H, W, bd, "smooth")
    pred = np.clip(org + rng.integers(-25, 26, org.shape), 0, mx).astype(np.int16)
    tus = tile(W, H, [(64, 64), (32, 32), (16, 16), (8, 8), (4, 4)], rng, [22, 27, 32, 37], bd)
    lv, asum, rec, coffs = oracle_chain(org, pred, tus, bd, W)
    d = _rc_descs(tus, W, coffs)
    n = len(tus)

    def launch(dev, outs):
        a = ops.resi_chain_batch(dev["org"], dev["pred"], outs[1], outs[0], _desc_dev(dev, "d"), n, bd, (0, mx))
        return [outs[0], outs[1], a]
    return Job("resi_chain_batch %dx%d" % (W, H), {"org": org, "pred": pred, "d": _plain(d)}, [lv, rec, asum],
               [np.full(lv.size, 0x5A5A5A5A, np.int32), pred.copy(), None], launch, ["vvcgpu_resi_chain_batch"])


def _resi_chain_runs_job(W, H):
    """vvcgpu_resi_chain_runs_batch: the class lists are ranges of the stream's identity array (vvcgpu_iota), the header a counter set.  Two sizes: the
    larger list outgrows the identity array the smaller one left on the stream (a new fill launch, the old array retired behind an event)"""
    from test_gpu_resichain import oracle_chain
    ops = _ops()
    rng = np.random.default_rng(31 + W)
    bd, mx = 10, 1023
    org = cases.rand_plane(rng, H, W, bd, "smooth")
    pred = np.clip(org + rng.integers(-25, 26, org.shape), 0, mx).astype(np.int16)
    tus = [(x, y, 16, 16, 0, 0, 32, 0, 0) for y in range(0, H // 2, 16) for x in range(0, W, 16)] + \
          [(x, y, 8, 8, 0, 0, 32, 0, 0) for y in range(H // 2, H, 8) for x in range(0, W, 8)]
    runs = [(16, 16, sum(t[2] == 16 for t in tus)), (8, 8, sum(t[2] == 8 for t in tus))]
    lv, asum, rec, coffs = oracle_chain(org, pred, tus, bd, W)
    d = _rc_descs(tus, W, coffs)
    n = len(tus)

    def launch(dev, outs):
        a = ops.resi_chain_runs_batch(dev["org"], dev["pred"], outs[1], outs[0], _desc_dev(dev, "d"), n, runs, bd, (0, mx))
        return [outs[0], outs[1], a]
    return Job("resi_chain_runs_batch %dx%d" % (W, H), {"org": org, "pred": pred, "d": _plain(d)}, [lv, rec, asum],
               [np.full(lv.size, 0x5A5A5A5A, np.int32), pred.copy(), None], launch, ["vvcgpu_resi_chain_runs_batch"])


def _transform_job():
    """vvcgpu_tr_fwd_batch followed by vvcgpu_dequant_tr_inv_batch on the same stream, each with 16384 TUs or more: only such lists reach the
    counter users of transform.hip (the forward transform then goes through the chain launch, the de-quantiser puts its TUs into class order on the
    device) -- two calls in a row take the two alternating counter sets.  The planes stay at 512x320: the forward TUs read the upper part twice (with
    different transform pairs, each to its own coefficients), the inverse TUs are 4x4 and 2x2."""
    ops = _ops()
    rng = np.random.default_rng(41)
    bd, W, H = 10, 512, 320
    resi = rng.integers(-300, 301, (H, W)).astype(np.int16)
    tr = [(y * W + x, 0, W, 4, 4, 0, 0, 0, 0) for y in range(0, 256, 4) for x in range(0, W, 4)]
    tr += [(y * W + x, 0, W, 4, 4, 1 + (x // 4 + y // 4) % 2, 1 + (x // 8) % 2, 0, 0) for y in range(0, 256, 4) for x in range(0, W, 4)]
    tr += [(y * W + x, 0, W, 16, 16, 0, 0, 0, 0) for y in range(256, H, 16) for x in range(0, W, 16)]
    tr = np.array(tr, dtype=ops.TR_DESC)
    tr["coeff_off"] = np.concatenate([[0], np.cumsum(tr["w"].astype(np.int64) * tr["h"])[:-1]])
    ncoef = int((tr["w"].astype(np.int64) * tr["h"]).sum())
    wcoef = np.full(ncoef, 7, np.int32)
    oracle().orc_tr_fwd_batch(p(resi), p(wcoef), p(tr), len(tr), bd)
    dq = [(y * W + x, 0, W, 4, 4, (x // 4) % 3, (y // 4) % 3, (x // 4 + y // 4) % 2, 0, int(rng.integers(10, 52))) for y in range(0, 256, 4) for x in range(0, W, 4)]
    dq += [(y * W + x, 0, W, 2, 2, 0, 0, (x // 2) % 2, 0, int(rng.integers(10, 52))) for y in range(256, H, 2) for x in range(0, W, 2)]
    dq = np.array(dq, dtype=ops.DQTR_DESC)
    dq["level_off"] = np.concatenate([[0], np.cumsum(dq["w"].astype(np.int64) * dq["h"])[:-1]])
    nlev = int((dq["w"].astype(np.int64) * dq["h"]).sum())
    assert len(tr) >= 16384 and len(dq) >= 16384 and nlev == W * H
    lv = (rng.integers(-30, 31, nlev) * (rng.random(nlev) < 0.35)).astype(np.int32)
    wres = np.full((H, W), 11, np.int16)
    wdq = np.full(nlev, 3, np.int32)
    oracle().orc_dequant_tr_inv_batch(p(lv), p(wres), p(dq), len(dq), bd, p(wdq))

    def launch(dev, outs):
        ops.tr_fwd_batch(dev["resi"], outs[0], _desc_dev(dev, "tr"), len(tr), bd)
        ops.dequant_tr_inv_batch(dev["lv"], outs[1], _desc_dev(dev, "dq"), len(dq), bd, outs[2])
        return outs
    return Job("tr_fwd_batch + dequant_tr_inv_batch", {"resi": resi, "tr": _plain(tr), "lv": lv, "dq": _plain(dq)}, [wcoef, wres, wdq],
               [np.full(ncoef, 7, np.int32), np.full((H, W), 11, np.int16), np.full(nlev, 3, np.int32)], launch,
               ["vvcgpu_tr_fwd_batch", "vvcgpu_dequant_tr_inv_batch"])


def _decaying_coef(rng, w, h, amp):
    yy, xx = np.mgrid[0:h, 0:w]
    return np.ascontiguousarray((rng.normal(0, amp, (h, w)) * np.exp(-(xx / w * 2 + yy / h * 2))).astype(np.int32).reshape(-1))


def _quant_job():
    """vvcgpu_quant_batch: its list of large TUs lives in scratch"""
    ops = _ops()
    rng = np.random.default_rng(51)
    bd = 10
    rows, coefs, off = [], [], 0
    for i in range(1200):
        w, h = [(4, 4), (8, 8), (16, 16), (32, 32), (64, 64), (16, 4), (8, 32), (2, 8)][i % 8] if i % 40 else (64, 64)
        rows.append((off, off, w, h, int(rng.integers(0, 2)), int(rng.integers(0, 2)), 0, int(rng.integers(12, 52)) + 12, 0))
        coefs.append(_decaying_coef(rng, w, h, 2500))
        off += w * h
    d = np.array(rows, dtype=ops.QUANT_DESC)
    coef = np.concatenate(coefs)
    wl, wsum = np.full(off, 9, np.int32), np.zeros(len(d), np.uint32)
    oracle().orc_quant_batch(p(coef), p(wl), p(d), len(d), bd, p(wsum))

    def launch(dev, outs):
        a = ops.quant_batch(dev["coef"], outs[0], _desc_dev(dev, "d"), len(d), bd)
        return [outs[0], a]
    return Job("quant_batch", {"coef": coef, "d": _plain(d)}, [wl, wsum], [np.full(off, 9, np.int32), None], launch, ["vvcgpu_quant_batch"])


def _depquant_job():
    """vvcgpu_depquant_batch: the workspace is the caller's (none of the library's per-stream state but the slot-free path; here for breadth)"""
    ops = _ops()
    rng = np.random.default_rng(17)
    rates = np.ascontiguousarray(np.load(os.path.join(G, "depquant.npz"))["rates"]).view(ops.DQ_RATES).reshape(-1)
    nt = len(rates)
    O = oracle()
    O.orc_depquant.restype = C.c_uint32
    descs, coefs, wants, sums, off = [], [], [], [], 0
    shapes = [(8, 8), (4, 4), (16, 8), (8, 16), (16, 16)]
    for i in range(150):
        w, h = shapes[i % len(shapes)]
        coef = _decaying_coef(rng, w, h, 1800)
        ri, qp, lam, luma = int((i * 37) % nt), int(rng.integers(10, 50)), float(rng.choice([5.0, 80.0, 900.0])), int(i % 3 != 0)
        lv = np.zeros(w * h, np.int32)
        sums.append(O.orc_depquant(p(coef), p(lv), w, h, luma, 10, qp, C.c_double(lam), C.c_void_p(rates.ctypes.data + ri * ops.DQ_RATES.itemsize)))
        descs.append((off, off, lam, qp, ri, w, h, luma, (0, 0, 0)))
        coefs.append(coef); wants.append(lv); off += w * h
    d = np.array(descs, dtype=ops.DEPQUANT_DESC)

    def launch(dev, outs):
        a = ops.depquant_batch(dev["coef"], outs[0], _desc_dev(dev, "d"), len(d), _desc_dev(dev, "rates"), off, 10)
        return [outs[0], a]
    return Job("depquant_batch", {"coef": np.concatenate(coefs), "d": _plain(d), "rates": _plain(rates)}, [np.concatenate(wants), np.array(sums, np.uint32)],
               [np.full(off, 9, np.int32), None], launch, ["vvcgpu_depquant_batch"])


def _tz_job():
    """vvcgpu_tz_search_batch: scratch claimed in tzsearch.hip (raster records) and, through it, in sadsearch.hip"""
    ops = _ops()
    rng = np.random.default_rng(10096)
    W, H, M, bd, n = 320, 256, 160, 10, 300
    org, ref_ = cases.tz_planes(rng, W, H, M, bd, motion=(11, -6))
    pus = cases.tz_pus(rng, n, W, H, M, [(8, 8), (16, 16), (32, 32), (64, 64), (16, 8), (8, 16), (32, 64), (64, 16)])
    cfg = cases.tz_cfg(W, H, M, 23.0, search_range=96, first_stop=1)
    want = np.zeros(n, cases.BEST)
    oracle().orc_tz_search(p(org), W, p(ref_), ref_.shape[1], p(pus), n, p(cfg), p(want))

    def launch(dev, outs):
        return [ops.tz_search_batch(dev["org"], dev["ref"], _desc_dev(dev, "pus"), n, cfg)]
    return Job("tz_search_batch", {"org": org, "ref": ref_, "pus": _plain(pus)}, [want], [None], launch, ["vvcgpu_tz_search_batch"])


def _affine_job():
    """vvcgpu_affine_pred_batch (bi-predictive PUs of the reference's affine fixture): scratch claimed in affine.hip, handed on to the motion compensation"""
    ops = _ops()
    g = np.load(os.path.join(G, "affine_mv.npz"))
    W, H, bd, M = 256, 128, 10, 144
    ref0 = np.ascontiguousarray(np.pad(g["Y"], M, mode="edge"))
    ref1 = np.ascontiguousarray(np.pad(np.random.default_rng(3).integers(0, 1024, (H, W)).astype(np.int16), M, mode="edge"))
    rows = g["rows"]
    pus = np.zeros(rows.shape[0], ops.AFFINE_PU)
    first, dst_off = 0, 0
    for i, r in enumerate(rows):
        px, py, w, h, six = r[:5]
        mv = np.zeros((2, 3, 2), np.int32); mv[0] = r[5:11].reshape(3, 2); mv[1] = rows[(i + 1) % len(rows)][5:11].reshape(3, 2)
        pus[i] = (px, py, w, h, six, i % 3 != 0, mv, dst_off, w, first)
        first += (w // 4) * (h // 4)
        dst_off += w * h
    first = int(first)
    wd = np.zeros(first, ops.MC_DESC)
    oracle().orc_affine_subblock_descs(p(pus), rows.shape[0], 0, W, H, 128, 128, M, M, ref0.shape[1], ref1.shape[1], p(wd))
    want = np.full(dst_off, -9, np.int16)
    oracle().orc_mc_batch(p(ref0), p(ref1), p(want), p(wd), first, bd, 0, 1023)

    def launch(dev, outs):
        ops.affine_pred_batch(dev["ref0"], dev["ref1"], outs[0], _desc_dev(dev, "pus"), rows.shape[0], first, 0, W, H, (M, M), ref0.shape[1], ref1.shape[1], bd, (0, 1023))
        return outs
    return Job("affine_pred_batch", {"ref0": ref0, "ref1": ref1, "pus": _plain(pus)}, [want], [np.full(dst_off, -9, np.int16)], launch, ["vvcgpu_affine_pred_batch"])


def _dist_job():
    """vvcgpu_dist_batch (SAD, blocks up to 128x128: the heavy list in scratch, a counter set as its length)"""
    from test_gpu_dist import make_descs
    ops = _ops()
    rng = np.random.default_rng(61)
    W, H, bd = 320, 256, 10
    org, cur = cases.rand_plane(rng, H, W, bd, "smooth"), cases.rand_plane(rng, H, W, bd, "smooth")
    d = make_descs(rng, W, H, ops.SAD, n_per_size=12)
    want = np.zeros(len(d), np.uint64)
    oracle().orc_dist_batch(ops.SAD, p(org), p(cur), p(d), len(d), p(want))

    def launch(dev, outs):
        return [ops.dist_batch(ops.SAD, dev["org"], dev["cur"], _desc_dev(dev, "d"), len(d), bd)]
    return Job("dist_batch", {"org": org, "cur": cur, "d": _plain(d)}, [want], [None], launch, ["vvcgpu_dist_batch"])


def _sad_search_job():
    """vvcgpu_sad_search with a motion-cost struct passed by pointer from the host (packed blocks in scratch)"""
    ops = _ops()
    rng = np.random.default_rng(71)
    bd, m, W, H, w, h, ss, nb = 10, 104, 256, 192, 32, 32, 1, 64
    dx0, dy0, nx, ny, sx, sy = -20, -15, 9, 7, 5, 5
    org = (2 * cases.rand_plane(rng, H, W, bd, "smooth").astype(np.int32) - cases.rand_plane(rng, H, W, bd, "smooth")).astype(np.int16)
    refp = cases.rand_plane(rng, H + 2 * m, W + 2 * m, bd, "smooth")
    blk = np.zeros(nb, ops.SEARCH_BLK)
    for i in range(nb):
        x, y = int(rng.integers(0, W - w)), int(rng.integers(0, H - h))
        blk[i] = (x, y, m + x + int(rng.integers(-6, 7)), m + y + int(rng.integers(-6, 7)))
    mv = ops.MvCost(37.5, -13, 22, 2, 0)
    want, wbest = np.zeros((nb, ny, nx), np.uint32), np.zeros(nb, ops.SEARCH_BEST)
    oracle().orc_sad_search(p(org), W, p(refp), W + 2 * m, p(blk), nb, w, h, ss, dx0, dy0, nx, ny, sx, sy, p(want), C.byref(mv), p(wbest))

    def launch(dev, outs):
        return list(ops.sad_search(dev["org"], dev["ref"], _desc_dev(dev, "blk"), nb, w, h, ss, dx0, dy0, nx, ny, sx, sy, ops.MvCost(37.5, -13, 22, 2, 0)))
    return Job("sad_search", {"org": org, "ref": refp, "blk": _plain(blk)}, [want, wbest], [None, None], launch, ["vvcgpu_sad_search"])


def _frac_job():
    """vvcgpu_frac_refine, 16x16 PUs with the Hadamard cost: the refinement's table image (and a motion-cost struct by pointer)"""
    ops = _ops()
    rng = np.random.default_rng(81)
    bd, mx, W, H, M, w, h, nb = 10, 1023, 256, 224, 16, 16, 16, 300
    ref = cases.rand_plane(rng, H + 2 * M, W + 2 * M, bd, "smooth")
    org = np.ascontiguousarray(np.clip(ref[M + 1:M + 1 + H, M + 2:M + 2 + W].astype(np.int32) + rng.integers(-6, 7, (H, W)), 0, mx).astype(np.int16))
    blk = np.zeros(nb, ops.FRAC_BLK)
    for i in range(nb):
        x, y, mvx, mvy = int(rng.integers(0, W - w + 1)), int(rng.integers(0, H - h + 1)), int(rng.integers(-3, 4)), int(rng.integers(-3, 4))
        blk[i] = (x, y, M + x + mvx, M + y + mvy, mvx, mvy)
    mv = ops.MvCost(17.0, 3, -2, 0, 0)
    want = np.zeros(nb, ops.FRAC_RESULT)
    oracle().orc_frac_refine(p(org), W, p(ref), W + 2 * M, p(blk), nb, w, h, bd, 0, mx, 1, C.byref(mv), p(want))

    def launch(dev, outs):
        return [ops.frac_refine(dev["org"], dev["ref"], _desc_dev(dev, "blk"), nb, w, h, bd, ops.MvCost(17.0, 3, -2, 0, 0), True, (0, mx))]
    return Job("frac_refine", {"org": org, "ref": ref, "blk": _plain(blk)}, [want], [None], launch, ["vvcgpu_frac_refine"])


def _sao_stats_job():
    """vvcgpu_sao_stats: a picture pass (ragged CTUs)"""
    ops = _ops()
    rng = np.random.default_rng(91)
    w, h, ctu, bd = 416, 240, 128, 10
    org, rec = cases.rand_plane(rng, h, w, bd, "smooth"), cases.rand_plane(rng, h, w, bd, "smooth")
    nx, ny = cases.n_ctus(w, h, ctu)
    want = np.zeros((nx * ny, 5, 2, 32), np.int64)
    oracle().orc_sao_stats(p(org), w, p(rec), w, w, h, ctu, ctu, bd, None, 5, 4, p(want))

    def launch(dev, outs):
        return [ops.sao_stats(dev["org"], dev["rec"], ctu, ctu, bd, None, 5, 4)]
    return Job("sao_stats", {"org": org, "rec": rec}, [want], [None], launch, ["vvcgpu_sao_stats"])


def _deblock_job():
    """vvcgpu_deblock: a picture pass with its configuration struct passed by pointer from the host"""
    ops = _ops()
    rng = np.random.default_rng(93)
    w, h, bd = 416, 240, 10
    Y, Cb, Cr = cases.rand_plane(rng, h, w, bd, "smooth"), cases.rand_plane(rng, h // 2, w // 2, bd, "smooth"), cases.rand_plane(rng, h // 2, w // 2, bd, "smooth")
    ev, eh, qpl, qpc = cases.deblock_maps(rng, w, h, "cu")
    wY, wCb, wCr = Y.copy(), Cb.copy(), Cr.copy()
    oracle().orc_deblock(p(wY), w, p(wCb), p(wCr), w // 2, w, h, p(ev), p(eh), p(qpl), p(qpc), C.byref(ops.deblock_cfg(bd, 1, -1, 2, -2)))

    def launch(dev, outs):
        ops.deblock(outs[0], outs[1], outs[2], dev["ev"], dev["eh"], dev["qpl"], dev["qpc"], ops.deblock_cfg(bd, 1, -1, 2, -2))
        return outs
    return Job("deblock", {"ev": ev, "eh": eh, "qpl": qpl, "qpc": qpc}, [wY, wCb, wCr], [Y, Cb, Cr], launch, ["vvcgpu_deblock"])


_TABLE = []


def job_table():
    """The jobs, built once per process (seeded: every build gives the same table).  Order: the small claims first, so that a young stream's scratch
    is outgrown several times on the way through the table (inside me_batch 6000, then by the residual chain's fall-back area)."""
    if not _TABLE:
        _TABLE.extend([_mc_job(8, 0), _me_job(64), _mc_job(10, 1), _dist_job(), _me_job(6000), _sad_search_job(), _mc_job(8, 1), _frac_job(),
                       _resi_chain_job(320, 128), _quant_job(), _resi_chain_runs_job(256, 128), _tz_job(), _resi_chain_runs_job(512, 320), _mc_job(10, 0),
                       _transform_job(), _affine_job(),
                       _sao_stats_job(), _resi_chain_job(448, 192), _depquant_job(), _deblock_job()])
    return _TABLE


def test_job_table_expectations_differ_from_the_initial_buffers():
    """No GPU: every output of every job has an expectation (from the oracle) that differs from what the output buffer holds in front of the call
    -- its `initial` contents, or, where the binding allocates the output itself, zeros and the POISON bytes written behind every use --
    so a call that wrote nothing cannot pass.  Jobs stay small: planes of 512x320 at the most."""
    table = job_table()
    assert len({j.name for j in table}) == len(table) >= 20
    for j in table:
        assert j.expected, j.name
        for i, (e, a) in enumerate(zip(j.expected, j.initial)):
            e8 = _plain(e).view(np.uint8).reshape(-1)
            assert e8.size > 0, (j.name, i)
            if a is None:
                assert np.any(e8 != POISON) and np.any(e8 != 0), (j.name, i)
                assert np.mean(e8 == POISON) < 0.5, (j.name, i)
            else:
                a8 = _plain(a).view(np.uint8).reshape(-1)
                assert a8.size == e8.size and not np.array_equal(a8, e8), (j.name, i)
        for v in j.inputs.values():
            if v.ndim == 2 and v.dtype == np.int16:                        # a plane: 512x320 with its search margins at the most
                assert v.shape[0] <= 320 + 2 * 160 and v.shape[1] <= 512 + 2 * 160, (j.name, v.shape)


# ---- the threaded test --------------------------------------------------------------------------------------------------------
CALLS_PER_PARAMETRISATION = 960          # rounds = this / (threads x calls of one pass over the table): a fixed count, no retry
RELEASE_EVERY = 3                        # rounds between two vvcgpu_stream_release + new stream of one thread
REJECT_THREAD, REJECT_ROUND = 1, 1       # who makes the one call the library refuses on the host, and when


def _new_stream(in_use, lock):
    """torch hands out its side streams from a pool, round-robin, so a new torch.cuda.Stream() may be the HIP stream another thread is driving right
    now -- which the contract (one host thread per stream at a time) forbids.  Draw until the handle is one no other thread holds; a handle that
    its last user has released (vvcgpu_stream_release returned) may be taken by any thread."""
    for _ in range(256):
        s = torch.cuda.Stream()
        with lock:
            if s.cuda_stream not in in_use:
                in_use.add(s.cuda_stream)
                return s
    raise RuntimeError("no free stream handle")


def _count_overlaps(intervals):
    """number of (call of thread a, call of thread b), a < b, whose [t0, t1] intervals intersect"""
    n = 0
    arr = [np.array(v, np.float64).reshape(-1, 2) for v in intervals]
    for a in range(len(arr)):
        for b in range(a + 1, len(arr)):
            if arr[a].size and arr[b].size:
                n += int(((arr[a][:, None, 0] < arr[b][None, :, 1]) & (arr[b][None, :, 0] < arr[a][:, None, 1])).sum())
    return n


@pytest.mark.gpu
@pytest.mark.parametrize("start", ["cold", "warm"])
@pytest.mark.parametrize("n_threads", [4, 8])
def test_concurrent_host_threads_match_oracle(n_threads, start):
    """n_threads host threads, each on its own torch stream with its own copies of every tensor, walk the job table `rounds` times from different
    offsets; after every call a thread waits for ITS stream only and compares bit for bit with the oracle.  Every RELEASE_EVERY rounds a thread
    releases its stream (vvcgpu_stream_release), drops it and goes on with a new one, so slots leave the table while others look theirs up.  One
    thread makes one call the library refuses on the host (bit depth 7): its error names that call, nobody else sees a failure.
    cold: after vvcgpu_shutdown -- the first calls race to build the table images and the slots; warm: after vvcgpu_warmup(8 / 10).
    The test must BE concurrent: at least one call of one thread overlaps in time a call of another (the count is printed)."""
    from vvcsoftware_vtm_amd import capi, ops
    table = job_table()
    calls_per_pass = sum(len(j.calls) for j in table)
    rounds = max(2, CALLS_PER_PARAMETRISATION // (n_threads * calls_per_pass))
    assert rounds > REJECT_ROUND
    assert type(capi.lib()) is C.CDLL                                      # ctypes.CDLL drops the GIL for the length of a call (PyDLL would not)
    torch.cuda.synchronize()
    if start == "cold":
        capi.call("vvcgpu_shutdown")
    else:
        capi.call("vvcgpu_warmup", 8)
        capi.call("vvcgpu_warmup", 10)
    barrier = threading.Barrier(n_threads, timeout=180)
    failures, lock = [], threading.Lock()
    intervals = [[] for _ in range(n_threads)]
    rejected, done, in_use = [], [False] * n_threads, set()

    def fail(msg):
        with lock:
            failures.append(msg)

    def timed(tid, fn, *a):
        t0 = time.perf_counter()
        try:
            return fn(*a)
        finally:
            intervals[tid].append((t0, time.perf_counter()))

    def worker(tid):
        try:
            s = _new_stream(in_use, lock)
            with torch.cuda.stream(s):
                mine = [j.upload() for j in table]
                s.synchronize()
            barrier.wait()
            for rnd in range(rounds):
                with torch.cuda.stream(s):
                    for k in range(len(table)):
                        if failures:
                            return
                        ji = (k + tid) % len(table)
                        j, (dev, init) = table[ji], mine[ji]
                        got = j.collect(timed(tid, j.launch, dev, j.fresh(init)))
                        for m in j.mismatches(got):
                            fail("thread %d round %d job '%s': %s" % (tid, rnd, j.name, m))
                    if tid == REJECT_THREAD and rnd == REJECT_ROUND:
                        tj = next(i for i, j in enumerate(table) if "vvcgpu_tr_fwd_batch" in j.calls)
                        dev, init = mine[tj]
                        try:
                            timed(tid, ops.tr_fwd_batch, dev["resi"], table[tj].fresh(init)[0], _desc_dev(dev, "tr"), 16, 7)
                            fail("thread %d: the call with bit depth 7 was not refused" % tid)
                        except capi.VvcGpuError as e:
                            rejected.append(str(e))
                    if (rnd + tid) % RELEASE_EVERY == RELEASE_EVERY - 1:
                        capi.call("vvcgpu_stream_release", C.c_void_p(s.cuda_stream))
                if (rnd + tid) % RELEASE_EVERY == RELEASE_EVERY - 1:
                    with lock:
                        in_use.discard(s.cuda_stream)
                    s = _new_stream(in_use, lock)                          # the old stream is dropped; its tensors stay (their work is complete)
            err = capi.lib().vvcgpu_last_error()                           # thread-local: only the refusing thread holds that text
            if (b"bit depth 7" in err) != (tid == REJECT_THREAD):
                fail("thread %d: vvcgpu_last_error() = %r" % (tid, err))
            capi.call("vvcgpu_stream_release", C.c_void_p(s.cuda_stream))
            done[tid] = True
        except BaseException as e:                                          # noqa: B902 -- everything goes into the list, the barrier must not be left waiting
            fail("thread %d: %s: %s" % (tid, type(e).__name__, e))
            barrier.abort()

    t_start = time.perf_counter()
    threads = [threading.Thread(target=worker, args=(i,), daemon=True, name="vvc-worker-%d" % i) for i in range(n_threads)]
    for t in threads:
        t.start()
    deadline = time.perf_counter() + 600
    for t in threads:
        t.join(max(0.0, deadline - time.perf_counter()))
    wall = time.perf_counter() - t_start
    hung = [t.name for t in threads if t.is_alive()]
    assert not hung, "threads still running after the time limit: %s; failures so far: %s" % (hung, failures[:20])
    assert not failures, "%d failure(s): %s" % (len(failures), failures[:20])
    assert all(done)
    assert len(rejected) == 1 and "vvcgpu_tr_fwd_batch" in rejected[0] and "tr_fwd_batch: bit depth 7" in rejected[0], rejected
    n_calls = sum(len(v) for v in intervals)
    overlaps = _count_overlaps(intervals)
    print("threads %d, %s start: %d rounds, %d library calls in %d timed launches, %d overlapping launch pairs between threads, %.1f s wall"
          % (n_threads, start, rounds, n_threads * rounds * calls_per_pass + 1, n_calls, overlaps, wall))
    assert n_calls >= n_threads * rounds * len(table)
    assert overlaps > 0, "no two calls of different threads overlapped in time: the test proved nothing"
    # nothing shared is left damaged: every job once more on the main thread's stream, then an orderly shutdown
    for j in table:
        dev, init = j.upload()
        bad = j.mismatches(j.run(dev, init))
        assert not bad, "after the threads, job '%s': %s" % (j.name, bad)
    torch.cuda.synchronize()
    assert capi.lib().vvcgpu_shutdown() == 0, capi.lib().vvcgpu_last_error()
