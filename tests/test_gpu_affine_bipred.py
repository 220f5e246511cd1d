"""vvcgpu_affine_bipred_me_batch on the device: whole affine bi-predictive searches (the bi-predictive part of InterSearch::xPredAffineInterSearch,
InterSearch.cpp:2823-2997) in one launch, against the compiled reference's results (tests/golden/affine_bipred.npz) and, call by call, against the
tests' restatement (tests/affine_bipred_cases.py, pinned to the reference by tests/test_affine_bipred_cpu.py).  All comparisons are exact."""
import functools
import itertools
import os

import numpy as np
import pytest

import affine_bipred_cases as ac
import pu_search_kit as kit
from vvcsoftware_vtm_amd import abi

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
W, H = 256, 128
PAIRS = list(itertools.product(ac.SIDES, ac.SIDES))          # every served (w, h); up to 1024 samples a wavefront owns the PU, above the workgroup


# ops.affine_bipred_cfg's parameters between pic_h and max_cu, as keys of ac.cfg_dict
CFG_FIELDS = ("bit_depth", "clp", "num_iter", "pick_list_by_cost", "mvd_l1_zero", "clip_key", "affine_type", "mvp_idx_cost")


def device_cfg(cfg, planes_dev, max_pu=(0, 0)):
    from vvcsoftware_vtm_amd import ops
    return kit.device_cfg(ops.affine_bipred_cfg, cfg, planes_dev, ac.MARGIN, CFG_FIELDS, max_pu)


def decode(res, trace):
    return kit.download(res, abi.AFFINE_BIPRED_RESULT), kit.download(trace, abi.AFFINE_BIPRED_STEP, (-1, abi.AFFINE_BIPRED_MAX_STEPS))


def run(org, planes, cfg, items, want_trace=True, max_pu=(0, 0)):
    from vvcsoftware_vtm_amd import ops
    return kit.run(ops.affine_bipred_me_batch, lambda d: device_cfg(cfg, d, max_pu), org, planes, items, want_trace, decode)


def shapes_of(n):
    """n shapes (w, h, six): the list of 96 holds every side pair six times, shuffled, so that wave- and workgroup-owned PUs alternate; the short lists
    straddle the four-wavefront-owners-per-workgroup boundary with both owner kinds"""
    rng = np.random.default_rng(n)
    if n == 96:
        shapes = PAIRS * 6
    else:
        shapes = [(16, 16), (64, 32), (32, 32), (16, 64), (128, 128)][:n]
    shapes = [shapes[int(i)] for i in rng.permutation(len(shapes))]
    return [(w, h, int(rng.integers(0, 2))) for w, h in shapes]


@functools.lru_cache(maxsize=None)
def fresh(n):
    """seeded inputs and the restatement's answer, computed once"""
    kw = {1: dict(num_iter=1, pick_list_by_cost=1), 3: dict(num_iter=1, mvd_l1_zero=1), 4: dict(clip_key=0), 5: dict(affine_type=0), 96: dict()}[n]
    org, planes, cfg, items = ac.fresh_set(900 + n, 8 if n in (3, 5) else 10, shapes_of(n), n_ref=(2, 2), **kw)
    res, trace = ac.search_all(org, planes, cfg, items)
    return org, planes, cfg, items, res, trace


@pytest.mark.parametrize("bd", [10, 8])
def test_results_and_trace_equal_the_reference_golden(bd):
    g = np.load(os.path.join(G, "affine_bipred.npz"))
    k = "bd%d_" % bd
    planes = kit.pad(g[k + "planes"])
    items, want, want_trace = g[k + "items"], g[k + "want"], g[k + "trace"]
    for cfg, idx in ac.golden_groups(g, bd):
        res, trace = run(g[k + "org"], planes, cfg, items[idx])
        for j, i in enumerate(idx):
            assert np.array_equal(trace[j], want_trace[i]), (bd, i, trace[j], want_trace[i])
            assert res[j].tobytes() == want[i].tobytes(), (bd, i, res[j], want[i])


@pytest.mark.parametrize("n", [1, 3, 4, 5, 96])
def test_results_and_trace_equal_the_restatement(n):
    org, planes, cfg, items, want, want_trace = fresh(n)
    if n == 96:
        px = items["w"].astype(int) * items["h"]
        assert set(zip(items["w"].tolist(), items["h"].tolist())) == set(PAIRS) and set(items["six_param"].tolist()) == {0, 1}
        assert (items["n_ref"] == 2).all()
        assert ((px[:-1] <= 1024) & (px[1:] > 1024)).any() and ((px[:-1] > 1024) & (px[1:] <= 1024)).any()     # the two owner kinds side by side
        # passes of the loop: the first always accepts (uiCostBi starts at the maximum), so an item stops in pass 2, 3 or 4 (or runs all four)
        ps = np.array([kit.passes(want_trace[i], want[i]["me_calls"]) for i in range(n)])
        assert set(ps.tolist()) == {2, 3, 4}
        stopped = [int(ps[i]) for i in range(n) if not want_trace[i][int(want[i]["me_calls"]) - 1]["accepted"]]
        assert {2, 3, 4} <= set(stopped)                                                                       # stops in pass 2, 3 and 4
    res, trace = run(org, planes, cfg, items)
    for i in range(n):
        assert np.array_equal(trace[i], want_trace[i]), (i, items[i]["w"], items[i]["h"], trace[i], want_trace[i])
        assert res[i].tobytes() == want[i].tobytes(), (i, res[i], want[i])


def test_max_pu_hint_gives_the_same_results_and_skips_what_exceeds_it():
    org, planes, cfg, items, want, want_trace = fresh(96)
    res, trace = run(org, planes, cfg, items, max_pu=(64, 32))
    big = (items["w"] > 64) | (items["h"] > 32)
    assert big.any() and (~big).any() and (items["w"][~big].astype(int) * items["h"][~big] > 1024).any()
    assert (res[big]["cost"] == np.uint64(kit.U64_MAX)).all() and (res[big]["me_calls"] == 0).all()
    assert trace[big].tobytes() == bytes(trace[big].nbytes)
    assert np.array_equal(res[~big], want[~big]) and np.array_equal(trace[~big], want_trace[~big])


def test_null_trace_gives_the_same_results():
    org, planes, cfg, items, want, _ = fresh(96)
    res, trace = run(org, planes, cfg, items[:24], want_trace=False)
    assert trace is None and np.array_equal(res, want[:24])


def test_items_outside_the_contract_get_the_sentinel():
    """one item per rule of the contract; the neighbours stay right"""
    org, planes, cfg, items, want, want_trace = fresh(96)
    items = items[:16].copy()
    items[1]["w"] = 24                           # no served side
    items[2]["h"] = 8                            # a side below 16
    items[3]["n_ref"][0] = 5
    items[4]["n_ref"][1] = 0
    items[5]["ref"][0][0]["plane"] = planes.shape[0]
    items[6]["ref"][1][0]["num_cand"] = 3
    items[7]["ref"][0][1]["num_cand"] = 0
    items[8]["pos_x"] = W - int(items[8]["w"]) + 4   # not inside the picture
    items[9]["pos_y"] = -4
    items[10]["ref_idx"][1] = 2                  # n_ref is 2
    items[11]["only_ref"][0] = 2
    items[12]["ref"][1][1]["mvp_idx"] = 2
    items[13]["org_stride"] = 0
    items[14]["only_ref"][1] = -2
    bad = list(range(1, 15))
    res, trace = run(org, planes, cfg, items)
    kit.sentinel_check(res, trace, (0, 15), bad, want, want_trace, abi.AFFINE_BIPRED_RESULT)
    # a side beyond the CTU: the same list under a CTU of 64
    cfg64 = dict(cfg, max_cu=64)
    sub = fresh(96)[3][:16]
    w64, t64 = ac.search_all(org, planes, cfg64, sub)
    beyond = (sub["w"] > 64) | (sub["h"] > 64)
    assert beyond.any() and (~beyond).any() and (w64[beyond]["cost"] == np.uint64(kit.U64_MAX)).all()
    res, trace = run(org, planes, cfg64, sub)
    assert np.array_equal(res, w64) and np.array_equal(trace, t64)


def test_two_streams_from_two_host_threads():
    from vvcsoftware_vtm_amd import ops
    org, planes, cfg, items, want, want_trace = fresh(96)
    d_org, d_planes, d_items = kit.dev(org), kit.dev(planes), ops.struct_to_device(items)
    dcfg = device_cfg(cfg, d_planes)
    kit.two_streams(lambda: ops.affine_bipred_me_batch(d_org, d_items, len(items), dcfg), decode, (want, want_trace))


def test_entry_equals_the_chained_form_of_the_existing_entries():
    """a consistency supplement, not evidence: affine_pred_batch -> pelop_batch -> affine_me_batch per iteration and reference index with host
    decisions between (tests/affine_bipred_chain.py) ends where the one-launch entry ends"""
    import affine_bipred_chain
    shapes = [(16, 16, 0), (32, 32, 1), (64, 32, 0), (16, 16, 1), (128, 128, 0), (32, 64, 1), (16, 128, 0), (16, 16, 0), (128, 16, 1), (32, 32, 0)]
    org, planes, cfg, items = ac.fresh_set(43, 10, shapes, n_ref=(2, 2))
    res, _ = run(org, planes, cfg, items)
    got, launches = affine_bipred_chain.chained(kit.dev(org), kit.dev(planes), cfg, items, ac.MARGIN)
    assert launches > 8
    for f in ("mv", "ref_idx", "mvp_idx", "mvp", "bits", "mot_bits", "me_calls", "closing", "cost"):
        assert np.array_equal(got[f], res[f]), (f, got[f], res[f])
