"""vvcgpu_affine_unipred_me_batch on the device: the uni-predictive part of InterSearch::xPredAffineInterSearch (InterSearch.cpp:2651-2814) for lists of
PUs, against the compiled reference's results (tests/golden/affine_unipred.npz) and the tests' restatement (tests/affine_unipred_cases.py, pinned to the
reference by tests/test_affine_unipred_cpu.py), and handed on to vvcgpu_affine_bipred_me_batch from device memory.  All comparisons are exact."""
import functools
import os

import numpy as np
import pytest
import torch

import affine_bipred_cases as ac
import affine_unipred_cases as uc
import pu_search_kit as kit
from vvcsoftware_vtm_amd import abi

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
W, H = 256, 128


# ops.affine_unipred_cfg's parameters between pic_h and max_cu, as keys of uc.cfg_dict
CFG_FIELDS = ("n_ref", "ref_plane", "bit_depth", "clp", "list1_to_list0", "fast_me_gen_b_low_delay", "mvd_l1_zero", "affine_type", "mvp_idx_cost")


def device_cfg(cfg, planes_dev, max_pu=None):
    from vvcsoftware_vtm_amd import ops
    return kit.device_cfg(ops.affine_unipred_cfg, cfg, planes_dev, uc.MARGIN, CFG_FIELDS, cfg["max_pu"] if max_pu is None else max_pu)


def decode(res, out):
    return kit.download(res, abi.AFFINE_UNIPRED_RESULT), kit.download(out, abi.AFFINE_BIPRED_ITEM)


def run(org, planes, cfg, items, want_items=True, max_pu=None):
    from vvcsoftware_vtm_amd import ops
    return kit.run(ops.affine_unipred_me_batch, lambda d: device_cfg(cfg, d, max_pu), org, planes, items, want_items, decode)


def same(got, want, items, what):
    for i in range(len(want)):
        assert got[i].tobytes() == want[i].tobytes(), (what, i, int(items[i]["w"]), int(items[i]["h"]), int(items[i]["six_param"]), got[i], want[i])


KW = {1: dict(n_ref=(1, 1)),
      3: dict(n_ref=(2, 2), mvd_l1_zero=1),
      4: dict(n_ref=(4, 2), list1_to_list0=(0, -1, -1, -1), fast_me_gen_b_low_delay=1),
      5: dict(n_ref=(1, 2), affine_type=0, list1_to_list0=(0, 0, -1, -1), fast_me_gen_b_low_delay=1, mvd_l1_zero=1),
      96: dict(n_ref=(2, 2), list1_to_list0=(-1, 1, -1, -1), fast_me_gen_b_low_delay=1)}


def shapes_of(n):
    """the list of 96 alternates wavefront- and workgroup-owned shapes and 4- / 6-parameter items; the short lists straddle the
    four-wavefront-owners-per-workgroup boundary with both owner kinds"""
    if n == 96:
        return uc.alternating_shapes(96)
    return [(16, 16, 1), (64, 32, 0), (32, 32, 0), (16, 64, 1), (128, 128, 1)][:n]


@functools.lru_cache(maxsize=None)
def fresh(n):
    """seeded inputs and the restatement's answer, computed once"""
    org, planes, cfg, items = uc.fresh_set(900 + n, 8 if n in (3, 5) else 10, shapes_of(n), **KW[n])
    facts = set()
    res, out = uc.search_all(org, planes, cfg, items, facts)
    return org, planes, cfg, items, res, out, facts


@pytest.mark.parametrize("bd", [10, 8])
def test_results_and_out_items_equal_the_reference_golden(bd):
    g = np.load(os.path.join(G, "affine_unipred.npz"))
    k = "bd%d_" % bd
    planes = kit.pad(g[k + "planes"])
    items, want, want_out = g[k + "items"], g[k + "want"], g[k + "out"]
    for cfg, idx in uc.golden_groups(g, bd):
        res, out = run(g[k + "org"], planes, cfg, items[idx])
        same(res, want[idx], items[idx], "result")
        same(out, want_out[idx], items[idx], "out-item")


@pytest.mark.parametrize("n", [1, 3, 4, 5, 96])
def test_results_and_out_items_equal_the_restatement(n):
    org, planes, cfg, items, want, want_out, facts = fresh(n)
    if n == 96:
        px = items["w"].astype(int) * items["h"]
        assert ((px[0::2] <= uc.WAVE_MAX).all() and (px[1::2] > uc.WAVE_MAX).all())             # the two owner kinds alternate
        assert {(int(w), int(h)) for w, h in zip(items["w"], items["h"])} == {(w, h) for w in uc.SIDES for h in uc.SIDES}
        for sel in (px <= uc.WAVE_MAX, px > uc.WAVE_MAX):
            assert set(items["six_param"][sel].tolist()) == {0, 1}
        assert {("start", 0), ("start", 1), ("start", 2), "six_skipped", "shortcut", "searched_l1", "shortcut_refused_six"} <= facts, facts
    res, out = run(org, planes, cfg, items)
    same(res, want, items, "result")
    same(out, want_out, items, "out-item")


@pytest.mark.parametrize("mvd_l1_zero", [0, 1])
def test_out_items_go_straight_into_the_affine_bipredictive_entry(mvd_l1_zero):
    """vvcgpu_affine_unipred_me_batch, then vvcgpu_affine_bipred_me_batch on the same stream with the first call's out-items as they lie in device
    memory: the outcome is that of the bi-predictive restatement on the uni-predictive restatement's out-items"""
    from vvcsoftware_vtm_amd import ops
    shapes = [(16, 16, 0), (32, 16, 1), (64, 64, 0), (16, 32, 1), (128, 32, 0), (32, 32, 1), (16, 64, 0), (64, 128, 1), (128, 128, 0), (64, 16, 1)]
    org, planes, cfg, items = uc.fresh_set(77 + mvd_l1_zero, 10, shapes, n_ref=(2, 2), mvd_l1_zero=mvd_l1_zero)
    for it in items:                                               # a 6-parameter PU whose 4-parameter search chose both lists
        if int(it["six_param"]) and int(it["only_ref"][1]) < 0:
            it["only_ref"][1] = 0
    want, want_items = uc.search_all(org, planes, cfg, items)
    bcfg = uc.bipred_cfg(cfg)
    want_bi, want_trace = ac.search_all(org, planes, bcfg, want_items)
    assert (want_bi["cost"] != np.uint64(kit.U64_MAX)).all() and (want_bi["me_calls"] >= 1).all()
    d_org, d_planes, m = kit.dev(org), kit.dev(planes), uc.MARGIN
    dbcfg = ops.affine_bipred_cfg(bcfg["lambda_"], [d_planes[i] for i in range(d_planes.shape[0])], (m, m), W, H, 10, (0, 1023), bcfg["num_iter"],
                                  bcfg["pick_list_by_cost"], mvd_l1_zero, bcfg["clip_key"], bcfg["affine_type"], bcfg["mvp_idx_cost"], bcfg["max_cu"])
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        res, out = ops.affine_unipred_me_batch(d_org, ops.struct_to_device(items), len(items), device_cfg(cfg, d_planes))
        bi, trace = ops.affine_bipred_me_batch(d_org, out, len(items), dbcfg)
    s.synchronize()
    same(res.cpu().numpy().view(abi.AFFINE_UNIPRED_RESULT), want, items, "result")
    same(out.cpu().numpy().view(abi.AFFINE_BIPRED_ITEM), want_items, items, "out-item")
    same(bi.cpu().numpy().view(abi.AFFINE_BIPRED_RESULT), want_bi, items, "bi-predictive result")
    assert np.array_equal(trace.cpu().numpy().view(abi.AFFINE_BIPRED_STEP).reshape(len(items), -1), want_trace)


def test_null_out_items_give_the_same_results():
    org, planes, cfg, items, want, _, _ = fresh(4)
    res, out = run(org, planes, cfg, items, want_items=False)
    assert out is None
    same(res, want, items, "result")


def test_p_slice_leaves_list_1_untouched():
    shapes = [(16, 16, 0), (64, 16, 1), (32, 64, 0), (128, 128, 1), (32, 32, 1)]
    org, planes, cfg, items = uc.fresh_set(5, 10, shapes, n_ref=(2, 0))
    want, want_out = uc.search_all(org, planes, cfg, items)
    for want_items in (True, False):
        res, out = run(org, planes, cfg, items, want_items=want_items)
        same(res, want, items, "result")
        assert (res["cost"][:, 1] == np.uint64(kit.U64_MAX)).all() and (res["cost"][:, 0] != np.uint64(kit.U64_MAX)).all()
        assert res["s"][:, 1].tobytes() == bytes(res["s"][:, 1].nbytes) and (res["valid_l1_cost"] == np.uint64(kit.U64_MAX)).all()
        if want_items:
            same(out, want_out, items, "out-item")
            assert (out["n_ref"][:, 1] == 0).all()


def test_max_pu_hint_gives_the_same_results_and_skips_what_exceeds_it():
    org, planes, cfg, items, want, want_out, _ = fresh(96)
    items, want, want_out = items[:24], want[:24], want_out[:24]
    res, out = run(org, planes, cfg, items, max_pu=(32, 16))
    big = (items["w"] > 32) | (items["h"] > 16)
    assert big.any() and (~big).any()
    assert (res[big]["cost"] == np.uint64(kit.U64_MAX)).all() and out[big].tobytes() == bytes(out[big].nbytes)
    assert np.array_equal(res[~big], want[~big]) and np.array_equal(out[~big], want_out[~big])
    res, out = run(org, planes, cfg, items, max_pu=(128, 64))                                  # both owner kinds, smaller tiles
    big = items["h"] > 64
    assert big.any() and (res[big]["cost"] == np.uint64(kit.U64_MAX)).all()
    assert np.array_equal(res[~big], want[~big]) and np.array_equal(out[~big], want_out[~big])


def test_items_outside_the_contract_get_the_sentinel():
    org, planes, cfg, items, want, want_out, _ = fresh(96)
    items = items[:13].copy()
    items[1]["w"] = 24                           # no served side
    items[2]["h"] = 256                          # above 128
    items[3]["w"] = 8                            # below 16
    items[4]["only_ref"][0] = 2                  # beyond list 0's references
    items[5]["only_ref"][1] = -2
    items[6]["ref"][1][0]["num_cand"] = 3
    items[7]["ref"][0][1]["num_cand"] = 0
    items[8]["pos_x"] = W - int(items[8]["w"]) + 4   # not inside the picture
    items[9]["org_stride"] = 0
    items[10]["pos_y"] = -4
    items[11]["pos_y"] = H - int(items[11]["h"]) + 4
    res, out = run(org, planes, cfg, items)
    for i in range(1, 12):
        assert not uc.item_ok(items[i], cfg), i
    kit.sentinel_check(res, out, (0, 12), range(1, 12), want, want_out, abi.AFFINE_UNIPRED_RESULT)


def test_two_streams_from_two_host_threads():
    from vvcsoftware_vtm_amd import ops
    org, planes, cfg, items, want, want_out, _ = fresh(96)
    items, want, want_out = items[:32], want[:32], want_out[:32]
    d_org, d_planes, d_items = kit.dev(org), kit.dev(planes), ops.struct_to_device(items)
    dcfg = device_cfg(cfg, d_planes)
    kit.two_streams(lambda: ops.affine_unipred_me_batch(d_org, d_items, len(items), dcfg), decode, (want, want_out))


def test_entry_ends_where_the_chain_of_the_existing_entries_ends():
    """a consistency supplement, not evidence: vvcgpu_affine_pred_batch + vvcgpu_dist_batch -> host -> vvcgpu_affine_me_batch per plane -> host
    (tests/affine_unipred_chain.py) ends where the entry ends"""
    import affine_unipred_chain
    shapes = [(16, 16, 0), (32, 16, 1), (64, 64, 0), (16, 16, 1), (128, 32, 0), (32, 32, 1), (16, 64, 0), (64, 128, 1), (16, 128, 1), (64, 16, 0), (32, 64, 1)]
    org, planes, cfg, items = uc.fresh_set(41, 10, shapes, n_ref=(2, 2), list1_to_list0=(-1, 0, -1, -1), fast_me_gen_b_low_delay=1, mvd_l1_zero=1)
    res, _ = run(org, planes, cfg, items)
    got, calls = affine_unipred_chain.chained(kit.dev(org), kit.dev(planes), cfg, items, uc.MARGIN)
    assert calls >= 4
    for f in res.dtype.names:
        assert np.array_equal(got[f], res[f]), (f, got[f], res[f])
