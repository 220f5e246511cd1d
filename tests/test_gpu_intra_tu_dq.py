"""vvcgpu_intra_tu_code_dq_batch on the device, bit for bit through the C ABI with the canaries intact: against the compiled reference's values
(tests/golden/intra_tu_dq.npz), and against the restatement of the pass (tests/intra_tu_dq_cases.py) on every shape, a random list with skipped items of every
kind, record counts around the trellis' packing, short lists, a list that gives every wavefront of every workgroup several items, a call of skipped items only, the hand-over from vvcgpu_intra_mode_cand_batch on one stream,
a workspace that is dirty and reused, all-zero items, the clip and the sibling's bound items; the seven-launch chain of the existing entries
(tests/intra_tu_dq_chain.py) and the sibling entry's stored prediction agree."""
import numpy as np
import pytest
import torch

import intra_mode_cand_cases as imc
import intra_mode_cand_chain
import intra_tu_code_cases as itc
import intra_tu_dq_cases as tdq
import intra_tu_dq_chain as chain
import rd_pass_kit as kit
from rd_pass_kit import dev
from vvcsoftware_vtm_amd import ops

pytestmark = pytest.mark.gpu

WS_FILL = 0xA7                                                               # the workspace holds anything on entry


def device_of(case):
    return chain.Device(case, WS_FILL)


def same(got, want):
    kit.same(got, want, chain.KEYS)


def cached(name, *args):
    return kit.cached(getattr(tdq, name), *args)


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("flags", [0, tdq.WRITE_PRED])
def test_against_golden(bd, flags):
    g = np.load(tdq.GOLDEN)
    case, _ = tdq.golden_case(g, bd)
    got = device_of(case).run(flags)
    k = "bd%d_want_" % bd
    for name in ("rec", "level", "abs_sum", "num_sig", "dist"):
        assert np.array_equal(got[name], g[k + name]), name
    assert np.array_equal(got["pred"], g[k + "pred"] if flags else case.tc.pred0)
    assert (got["mode_out"] == np.where(case.tc.items["mode"] >= 0, case.tc.items["mode"], -1)).all()


@pytest.mark.parametrize("bd", [8, 10])
def test_every_shape_at_an_odd_position_and_odd_strides(bd):
    case, want = cached("shapes_case", bd)
    D = device_of(case)
    same(D.run(), want)
    got = D.run(use_pred=False)                                              # no PRED_GIVEN item, no WRITE_PRED: the prediction buffer may be absent
    got["pred"] = want["pred"]
    same(got, want)


@pytest.mark.parametrize("bd", [8, 10])
def test_random_list_with_skipped_items_of_every_kind(bd):
    case, lists, want = cached("random_case", bd)
    D = device_of(case)
    ml = dev(lists)
    same(D.run(0, ml), want)                                                 # the markers of the skipped items, nothing of theirs touched in the three buffers
    same(D.run(tdq.WRITE_PRED, ml), tdq.restate(case, tdq.WRITE_PRED, mode_list=lists))
    same(D.run(0, None), tdq.restate(case, mode_list=None))                  # without mode_list every FROM_LIST item is skipped, nothing else changes


@pytest.mark.parametrize("served", [1, 15, 16, 17, 63, 64, 65])
def test_record_counts_around_the_trellis_packing(served):
    case, want = cached("count_case", served)
    same(device_of(case).run(), want)
    assert (want["abs_sum"] != tdq.U32_MAX).sum() == served


def compute_units():
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


def test_every_wavefront_of_every_workgroup_walks_several_items():
    """27 items per compute unit and 88 more (7000 on an MI355X): the front and the back run all twelve wavefronts of every workgroup, each over two or
    three items with skipped ones among them, so the LDS slice of every wavefront, its run in the work list from one atomic add for several items, and the
    tile's reuse from item to item are all in the comparison"""
    cus = compute_units()
    case, lists, want = cached("waves_case", cus)
    tdq.check_waves(case, want, cus)
    same(device_of(case).run(0, dev(lists)), want)


def test_list_lengths_around_the_workgroup_and_wavefront_counts():
    """the items are dealt to the workgroups first and to their wavefronts then: the lengths at which a workgroup's second wavefront gets its first item
    (one more than the compute units) and a wavefront its second (one more than twelve times as many), and the two below each"""
    cus = compute_units()
    case, lists, want = cached("waves_case", cus)
    D, ml = device_of(case), dev(lists)
    for m in tdq.wave_lengths(cus):
        same(D.run(0, ml, n=m), tdq.prefix_of(case, want, m))


def test_short_lists_and_a_shuffled_order():
    """list lengths 1 .. 9 (a workgroup of its own for every item); n == 0 touches nothing"""
    case, want = cached("shapes_case", 10)
    assert device_of(case).run(n=0)["rec"].tobytes() == case.tc.initial()[1].tobytes()
    perm = np.random.default_rng(12).permutation(len(case.tc.items))
    for n in range(1, 10):
        sub = case.sub(perm[:n])
        same(device_of(sub).run(), tdq.restate(sub))
    got = device_of(case.sub(perm)).run()
    for k in ("abs_sum", "num_sig", "dist", "mode_out"):
        assert np.array_equal(got[k], want[k][perm]), k
    for k in ("pred", "rec", "level"):
        assert np.array_equal(got[k], want[k]), k


def test_a_call_of_skipped_items_only():
    """markers everywhere, the buffers untouched; the trellis launch leaves on a zero count"""
    case, want = cached("all_skipped_case")
    got = device_of(case).run(tdq.WRITE_PRED)
    same(got, want)
    assert (got["abs_sum"] == tdq.U32_MAX).all() and (got["num_sig"] == tdq.U32_MAX).all() and (got["dist"] == tdq.U64_MAX).all() and (got["mode_out"] == -1).all()


@pytest.mark.parametrize("bd", [8, 10])
def test_handover_from_intra_mode_cand_batch(bd):
    """vvcgpu_intra_mode_cand_batch, then the entry with mode_list = its list_out and refs_base = the references it gathered, on one stream with no
    synchronisation between; slots beyond a PU's list are skipped"""
    base, cand, case, want = cached("handover_case", bd)
    M = intra_mode_cand_chain.Device(base)
    refs = M.fresh_refs()
    D = chain.Device(case, WS_FILL, refs=refs, org=M.org)
    pred, rec, level = D.fresh()
    _, lists, _ = intra_mode_cand_chain.run_entry(M, imc.USE_MPM, 23.75, refs)
    out = D.launch(pred, rec, level, 0, lists)
    got = kit.download((pred, rec, level) + out, chain.KEYS)
    assert np.array_equal(lists.cpu().numpy(), cand["lists"])
    same(got, want)
    skipped = want["abs_sum"] == tdq.U32_MAX
    assert skipped.any() and (got["mode_out"][skipped] == -1).all() and (got["mode_out"][~skipped] >= 0).all()


def test_workspace_dirty_and_reused():
    """a workspace prefilled with a byte pattern serves a list with 64x64, 64x16 and 16x64 items, then a different list at the same level offsets: a zeroed
    high-frequency region that was not written, or a history block read before it was written, shows in the second run at the latest"""
    (c1, w1), (c2, w2) = cached("workspace_cases")
    D1, D2 = device_of(c1), device_of(c2)
    ws = torch.full((max(D1.ws.numel(), D2.ws.numel()),), WS_FILL, dtype=torch.uint8, device="cuda")
    for D, want in ((D1, w1), (D2, w2), (D1, w1)):
        same(D.run(ws=ws), want)


@pytest.mark.parametrize("bd", [8, 10])
def test_all_zero_items(bd):
    """pred == org, and a flat residual just under the trellis' last threshold: abs_sum 0, num_sig 0, rec == clip(pred), dist == SSE(org, clip(pred))"""
    case, want = cached("zero_case", bd)
    got = device_of(case).run()
    same(got, want)
    tdq.check_zero(case, got)


@pytest.mark.parametrize("bd", [8, 10])
def test_clip_and_bounds(bd):
    """a narrowed clip range; predictions at the clip bounds with the original just inside; the sibling's bound items"""
    mx = (1 << bd) - 1
    case, _ = cached("shapes_case", bd)
    clp = (mx // 8, mx - mx // 5)
    same(device_of(case).run(tdq.WRITE_PRED, clp=clp), tdq.restate(case, tdq.WRITE_PRED, clp))
    case, want = cached("clip_case", bd)
    same(device_of(case).run(), want)
    for inverse in (False, True):
        case, want = tdq.with_dq(itc.checker(bd, inverse), bd)
        same(device_of(case).run(), want)
    assert bd != 10 or int(want["dist"][0]) > 1 << 31
    case, want = tdq.with_dq(itc.bounds_case(bd), bd)
    same(device_of(case).run(), want)


def test_chain_of_the_existing_entries_agrees():
    """the seven launches of the existing entries (vvcgpu_depquant_batch in the middle, dep_quant = 1 behind it) give the entry's levels, abs_sum,
    reconstruction and distortion (and prediction, under WRITE_PRED)"""
    case = cached("chain_case")
    D = device_of(case)
    C = chain.Chain(D.d_host, D.t_host, case.dq, D.rates, case.tc.level_size, case.bd, D.refs, D.org)
    p1, r1, l1 = D.fresh()
    p2, r2, l2 = D.fresh()
    abs_c, dist_c = C.run(p1, r1, l1)
    abs_e, _, dist_e, _ = D.launch(p2, r2, l2, tdq.WRITE_PRED)
    torch.cuda.synchronize()
    assert torch.equal(abs_c, abs_e) and torch.equal(dist_c, dist_e) and torch.equal(p1, p2) and torch.equal(r1, r2) and torch.equal(l1, l2)
    assert int((abs_e != 0).sum()) * 2 >= D.n


@pytest.mark.parametrize("bd", [8, 10])
def test_write_pred_stores_the_sibling_entrys_prediction(bd):
    """WRITE_PRED stores exactly what vvcgpu_intra_tu_code_batch stores for the same items; without the flag pred_base keeps its canaries"""
    case, lists, want = cached("random_case", bd)
    D = device_of(case)
    ml = dev(lists)
    got = D.run(tdq.WRITE_PRED, ml)
    pred, rec, _ = D.fresh()
    level = torch.zeros(case.tc.level_size + 64 * 64 + 16, dtype=torch.int32, device="cuda")    # (the sibling also serves the item whose levels leave the extent)
    ops.intra_tu_code_batch(D.refs, D.preds, D.org, pred, rec, level, D.tus, D.n, ml, tdq.WRITE_PRED, bd, (0, (1 << bd) - 1))
    torch.cuda.synchronize()
    sib = pred.cpu().numpy()
    # (the sibling has no rule on level offsets, rate tables or lambdas: the items only this entry skips keep their canaries here)
    for i, it in enumerate(case.tc.items):
        r = itc.resolve(case.tc, i, tdq.WRITE_PRED, lists)
        if r is None or r[0] < 0 or tdq.resolve(case, i, tdq.WRITE_PRED, lists) is not None:
            continue
        itc.block(sib, int(it["pred_off"]), int(it["pred_stride"]), int(it["w"]), int(it["h"]))[:] = itc.PRED_CANARY
    assert np.array_equal(got["pred"], sib) and not np.array_equal(sib, case.tc.pred0)
    assert np.array_equal(D.run(0, ml)["pred"], case.tc.pred0)
