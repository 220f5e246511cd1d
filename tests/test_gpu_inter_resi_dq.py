"""vvcgpu_inter_resi_code_dq_batch on the device, bit for bit through the C ABI with the canaries intact: against the compiled reference's values
(tests/golden/inter_resi_dq.npz), and against the restatement of the pass (tests/inter_resi_dq_cases.py) on every shape, a random list with skipped items,
record counts around the trellis' packing, the hand-over from vvcgpu_merge_cand_batch on one stream, a workspace that is dirty and reused, all-zero slots,
predictions at the clip bounds; as a supplement the chain of the existing entries (tests/inter_resi_dq_chain.py); the contract of the argument checks.  The harness this file shares
with tests/test_gpu_inter_resi_code.py is beside Device in tests/inter_resi_code_chain.py."""
import numpy as np
import pytest
import torch

import inter_resi_code_cases as irc
import inter_resi_dq_cases as dqc
import inter_resi_dq_chain as chain
import merge_cand_chain
import rd_pass_kit as kit
from vvcsoftware_vtm_amd import capi

pytestmark = pytest.mark.gpu

WS_FILL = 0xA7                                                               # the workspace holds anything on entry


def device_of(case):
    return chain.Device(case.bd, case.org, case.pred, case.items, case.dq, case.rates, case.cand_size, case.level_size, chain.FILLS, WS_FILL)


def run(case, flags=0, rd_list=None, D=None, with_rec=None):
    return (D or device_of(case)).run(flags, rd_list, with_rec)


def same(got, want):
    kit.same(got, want, chain.KEYS)


def cached(name, *args):
    return kit.cached(getattr(dqc, name), *args)


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("flags", [0, dqc.WRITE_REC])
def test_against_golden(bd, flags):
    g = np.load(dqc.GOLDEN)
    case = dqc.golden_case(g, bd)
    got = run(case, flags)
    k = "bd%d_want_" % bd
    for name in ("abs_sum", "zero_dist", "dist_resi", "dist_rec", "level", "resi"):
        assert np.array_equal(got[name], g[k + name]), name
    assert np.array_equal(got["rec"], g[k + "rec"] if flags else np.full(case.cand_size, irc.REC_CANARY, np.int16))


@pytest.mark.parametrize("bd", [8, 10])
def test_every_shape_at_an_odd_position_and_stride(bd):
    case, want = cached("shapes_case", bd)
    assert {(int(w), int(h)) for w, h in zip(case.items["w"], case.items["h"])} == set(dqc.all_shapes())
    same(run(case), want)
    same(run(case, dqc.WRITE_REC), dqc.restate(case, dqc.WRITE_REC))


@pytest.mark.parametrize("bd", [8, 10])
def test_random_list_with_skipped_items(bd):
    case, rows, want = cached("random_case", bd)
    D = device_of(case)
    rd = chain.dev(rows)
    same(run(case, 0, rd, D), want)                                          # the markers of the skipped items and slots, nothing touched in the three buffers
    same(run(case, dqc.WRITE_REC, rd, D), dqc.restate(case, dqc.WRITE_REC, rd_list=rows))
    # without rd_list every list item is skipped, nothing else changes; a rec_base that is given without WRITE_REC stays untouched
    same(run(case, 0, None, D, with_rec=True), dqc.restate(case, 0, rd_list=None))


@pytest.mark.parametrize("served", [1, 15, 16, 17, 63, 64, 65])
def test_record_counts_around_the_trellis_packing(served):
    case, want = cached("count_case", served)
    same(run(case, dqc.WRITE_REC), dqc.restate(case, dqc.WRITE_REC))
    assert (want["abs_sum"] != dqc.U32_MAX).sum() == served


def test_a_call_of_skipped_items_only():
    case, want = cached("all_skipped_case")
    same(run(case, dqc.WRITE_REC), want)


@pytest.mark.parametrize("bd", [8, 10])
def test_handover_from_merge_cand_batch(bd):
    """vvcgpu_merge_cand_batch, then the entry with list items for slots 0 .. 3 on the same stream, no download in between"""
    fr, L, mwant, case, want = cached("handover_case", bd)
    M = merge_cand_chain.Device(fr, L)
    D = chain.Device(bd, fr.org, np.zeros(1, np.int16), case.items, case.dq, case.rates, case.cand_size, case.level_size, chain.FILLS, WS_FILL)
    got, rd, _ = D.handover(M, len(case.pred))
    assert np.array_equal(rd, mwant["rd_list"])
    same(got, want)


def test_workspace_dirty_and_reused():
    """a workspace prefilled with a byte pattern serves a list with 64x64, 64x16 and 16x64 items, then a different list: a zeroed high-frequency region that
    was not written, or a history block read before it was written, shows in the second run at the latest"""
    (c1, w1), (c2, w2) = cached("workspace_cases")
    D1, D2 = device_of(c1), device_of(c2)
    n_ws = max(D1.ws.numel(), D2.ws.numel())
    ws = torch.full((n_ws,), WS_FILL, dtype=torch.uint8, device="cuda")
    for D, want in ((D1, w1), (D2, w2), (D1, w1)):
        resi, rec, level = D.fresh()
        same(D.collect(resi, rec, level, D.run_entry(resi, None, level, 0, None, ws=ws)), want)


@pytest.mark.parametrize("bd", [8, 10])
def test_all_zero_slots(bd):
    """pred == org, and a residual just under the trellis' last threshold: resi' stored as zeros, dist_resi == zero_dist"""
    case, want = cached("zero_case", bd)
    got = run(case, dqc.WRITE_REC)
    same(got, want)
    chain.check_all_zero_slots(case.items, got)


@pytest.mark.parametrize("bd", [8, 10])
def test_prediction_at_the_clip_bounds(bd):
    case, want = cached("clip_case", bd)
    served = want["abs_sum"] != dqc.U32_MAX
    assert (want["dist_rec"][served] != want["dist_resi"][served]).any()     # the clip is exercised
    same(run(case), want)
    same(run(case, dqc.WRITE_REC), dqc.restate(case, dqc.WRITE_REC))


def test_chain_of_the_existing_entries_agrees():
    """the eight launches of the existing entries (vvcgpu_depquant_batch in the middle, dep_quant = 1 behind it) give the entry's numbers and buffers"""
    case = cached("chain_case")
    D = device_of(case)
    C = chain.Chain(D)
    r1, c1, l1 = D.fresh()
    r2, c2, l2 = D.fresh()
    out_c = C.run(r1, c1, l1)
    out_e = D.run_entry(r2, c2, l2, dqc.WRITE_REC)
    torch.cuda.synchronize()
    assert C.same(out_c, out_e) and torch.equal(r1, r2) and torch.equal(c1, c2) and torch.equal(l1, l2)


def test_contract():
    """n == 0 is a no-op; every VVCGPU_E_ARG case and an unserved quantiser leave the outputs and the buffers untouched"""
    case, _ = cached("count_case", 17)
    D = device_of(case)
    resi, rec, level = D.fresh()
    n = D.n
    outs = [torch.full((n, 6), 77, dtype=torch.int32, device="cuda")] + [torch.full(s, 77, dtype=torch.int64, device="cuda") for s in ((n, 6), (n, 6), (n,))]
    before = [t.clone() for t in (resi, rec, level, *outs)]

    def call(**kw):
        a = dict(org=D.org, pred=D.pred, items=D.items_dev, dq=D.dq_dev, n=n, rates=D.rates_dev, n_rates=len(D.rates), quantiser=dqc.Q_DEPQUANT, resi=resi,
                 rec=rec, level=level, extent=D.level_size, flags=0, cmin=0, cmax=1023, abs_sum=outs[0], ws=D.ws, ws_ptr=None, ws_bytes=D.ws.numel())
        a.update(kw)
        ws_ptr = a["ws_ptr"] if a["ws_ptr"] is not None else capi.ptr(a["ws"])
        return capi.lib().vvcgpu_inter_resi_code_dq_batch(capi.ptr(a["org"]), capi.ptr(a["pred"]), capi.ptr(a["items"]), capi.ptr(a["dq"]), a["n"], None,
                                                          capi.ptr(a["rates"]), a["n_rates"], a["quantiser"], capi.ptr(a["resi"]), capi.ptr(a["rec"]),
                                                          capi.ptr(a["level"]), a["extent"], a["flags"], case.bd, a["cmin"], a["cmax"], capi.ptr(a["abs_sum"]),
                                                          capi.ptr(outs[1]), capi.ptr(outs[2]), capi.ptr(outs[3]), ws_ptr, a["ws_bytes"], None)

    assert call(n=0) == 0
    for kw in (dict(org=None), dict(items=None), dict(dq=None), dict(rates=None), dict(level=None), dict(abs_sum=None), dict(ws=None),
               dict(ws_bytes=capi.lib().vvcgpu_inter_resi_code_dq_workspace_bytes(D.level_size, n) - 1), dict(ws_ptr=D.ws.data_ptr() + 8), dict(flags=4),
               dict(flags=dqc.WRITE_REC, rec=None), dict(cmin=9, cmax=3), dict(cmax=1 << 16)):
        assert call(**kw) == -1, kw
    for q in (0, 2):
        assert call(quantiser=q) == -3
    torch.cuda.synchronize()
    for t, b in zip((resi, rec, level, *outs), before):
        assert torch.equal(t, b)
    assert call() == 0                                                       # and the same arguments unchanged are served
    torch.cuda.synchronize()
    assert not torch.equal(outs[0], before[3])
