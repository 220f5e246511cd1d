"""vvcgpu_inter_resi_code_batch on the device, bit for bit through the C ABI with the canaries intact: against the compiled reference's values
(tests/golden/inter_resi_code.npz), and against the restatement of the pass (tests/inter_resi_code_cases.py) on every shape, a random list, the hand-over
from vvcgpu_merge_cand_batch on one stream, all-zero slots, the bounds and predictions at the clip bounds; as a supplement the chain of the existing
entries (tests/inter_resi_code_chain.py, which also holds the harness this file shares with tests/test_gpu_inter_resi_dq.py)."""
import numpy as np
import pytest
import torch

import inter_resi_code_cases as irc
import inter_resi_code_chain as chain
import merge_cand_chain
import rd_pass_kit as kit

pytestmark = pytest.mark.gpu


def device_of(case):
    return chain.Device(case.bd, case.org, case.pred, case.items, case.cand_size, case.level_size, chain.FILLS)


def run(case, flags=0, rd_list=None, D=None, with_rec=None):
    return (D or device_of(case)).run(flags, rd_list, with_rec)


def same(got, want):
    kit.same(got, want, chain.KEYS)


def cached(name, *args):
    return kit.cached(getattr(irc, name), *args)


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("flags", [0, irc.WRITE_REC])
def test_against_golden(bd, flags):
    g = np.load(irc.GOLDEN)
    case = irc.golden_case(g, bd)
    got = run(case, flags)
    k = "bd%d_want_" % bd
    for name in ("abs_sum", "zero_dist", "dist_resi", "dist_rec", "level", "resi"):
        assert np.array_equal(got[name], g[k + name]), name
    assert np.array_equal(got["rec"], g[k + "rec"] if flags else np.full(case.cand_size, irc.REC_CANARY, np.int16))


@pytest.mark.parametrize("bd", [8, 10])
def test_every_shape_at_an_odd_position(bd):
    case, want = cached("shapes_case", bd)
    assert {(int(w), int(h)) for w, h in zip(case.items["w"], case.items["h"])} == set(irc.all_shapes())
    same(run(case), want)
    same(run(case, irc.WRITE_REC), irc.restate(case, irc.WRITE_REC))


@pytest.mark.parametrize("bd", [8, 10])
def test_random_list(bd):
    case, rows, want = cached("random_case", bd)
    D = device_of(case)
    rd = chain.dev(rows)
    same(run(case, 0, rd, D), want)
    same(run(case, irc.WRITE_REC, rd, D), irc.restate(case, irc.WRITE_REC, rd_list=rows))
    # without rd_list every list item is skipped, nothing else changes; a rec_base that is given without WRITE_REC stays untouched
    same(run(case, 0, None, D, with_rec=True), irc.restate(case, 0, rd_list=None))


@pytest.mark.parametrize("bd", [8, 10])
def test_handover_from_merge_cand_batch(bd):
    """vvcgpu_merge_cand_batch, then the entry with list items for slots 0 .. 3 on the same stream, no download in between"""
    fr, L, mwant, case, want = cached("handover_case", bd)
    M = merge_cand_chain.Device(fr, L)
    D = chain.Device(bd, fr.org, np.zeros(1, np.int16), case.items, case.cand_size, case.level_size, chain.FILLS)
    got, rd, pred = D.handover(M, len(case.pred))
    assert np.array_equal(rd, mwant["rd_list"])
    assert np.array_equal(pred[:len(mwant["pred"])], mwant["pred"])
    same(got, irc.restate(case, irc.WRITE_REC, rd_list=mwant["rd_list"]))
    assert np.array_equal(got["abs_sum"], want["abs_sum"])


@pytest.mark.parametrize("bd", [8, 10])
def test_all_zero_slots(bd):
    case, want = cached("zero_case", bd)
    got = run(case, irc.WRITE_REC)
    same(got, irc.restate(case, irc.WRITE_REC))
    chain.check_all_zero_slots(case.items, got)


@pytest.mark.parametrize("bd", [8, 10])
def test_bounds(bd):
    mx = (1 << bd) - 1
    case, want = cached("checker_case", bd)
    got = run(case, irc.WRITE_REC)
    same(got, irc.restate(case, irc.WRITE_REC))
    assert int(got["zero_dist"][0]) == int(got["zero_dist"][1]) == 64 * 64 * mx * mx
    for v in (mx, -mx):
        case, want = irc.flat_case(bd, v)
        same(run(case), want)


@pytest.mark.parametrize("bd", [8, 10])
def test_prediction_at_the_clip_bounds(bd):
    case, want = cached("clip_case", bd)
    served = want["abs_sum"] != irc.U32_MAX
    assert (want["dist_rec"][served] != want["dist_resi"][served]).any()     # the clip is exercised
    same(run(case), want)
    same(run(case, irc.WRITE_REC), irc.restate(case, irc.WRITE_REC))


def test_chain_of_the_existing_entries_agrees():
    """the eight launches of the existing entries give the entry's numbers and buffers (every shape, DCT-II and the EMT pairs where the sides allow them)"""
    rng = np.random.default_rng(77)
    plane = irc.fresh_plane(rng, 10)
    specs = []
    for k, (w, h) in enumerate(irc.all_shapes()):
        x, y = irc.place(rng, w, h)
        specs.append(dict(x=x, y=y, w=w, h=h, qp=(22, 27, 32, 37)[k % 4] + 12, tr=[0] + (list(irc.EMT) if 4 <= w <= 32 and 4 <= h <= 32 else [])))
    case = irc.make(10, plane, specs, rng)
    D = device_of(case)
    C = chain.Chain(D)
    r1, c1, l1 = D.fresh()
    r2, c2, l2 = D.fresh()
    out_c = C.run(r1, c1, l1)
    out_e = D.run_entry(r2, c2, l2, irc.WRITE_REC)
    torch.cuda.synchronize()
    assert C.same(out_c, out_e) and torch.equal(r1, r2) and torch.equal(c1, c2) and torch.equal(l1, l2)
