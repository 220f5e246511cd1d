"""vvcgpu_resi_rate_batch and vvcgpu_inter_resi_choose_batch on the device, bit for bit through the C ABI: against the compiled reference's values
(tests/golden/resi_rate.npz), against the restatement (tests/resi_rate_cases.py) on random blocks with random context rows and on a list longer than
the grid, the skip markers with the canaries of ctx_out intact, and the three-call chain behind vvcgpu_inter_resi_code_batch / _dq_batch on one stream."""
import numpy as np
import pytest

import inter_resi_code_cases as irc
import inter_resi_code_chain
import inter_resi_dq_cases as dqc
import inter_resi_dq_chain
import rd_pass_kit as kit
import resi_rate_cases as rrc
import resi_rate_chain as chain
from vvcsoftware_vtm_amd import abi

pytestmark = pytest.mark.gpu


def golden_model():
    g = rrc.golden()
    return g, chain.Model(g["est_bits"], g["next_state"])


def same_rate(got, want, keys=("frac_bits", "num_sig", "ctx_out")):
    kit.same(got, want, keys)


def test_rate_against_golden():
    g, M = golden_model()
    items = np.ascontiguousarray(g["items"]).view(abi.RESI_RATE_ITEM).reshape(-1)
    got = chain.run_rate(M, g["level"], items, g["ctx_before"])
    same_rate(got, dict(frac_bits=g["bits"], num_sig=g["num_sig"], ctx_out=g["ctx_after"]))


def test_choose_against_golden():
    g = rrc.golden()
    c = {k[len("choose_"):]: g[k] for k in g.files if k.startswith("choose_") and not k.startswith("choose_out_")}
    c["weight"], c["scale"] = c["weight"].view(np.float64), float(c["scale"].view(np.float64)[0])
    want = {k: g["choose_out_" + k] for k in chain.CHOOSE_KEYS}
    want["min_cost"] = want["min_cost"].view(np.float64)
    chain.same_choose(chain.run_choose(c), want)


def random_rate_case(seed, count):
    g = rrc.golden()
    level, items, ctx = rrc.random_list(seed, count)
    return level, items, ctx, chain.want_rate(level, items, None, ctx, g["est_bits"], g["next_state"])


@pytest.mark.parametrize("seed", [11, 19])
def test_rate_random_blocks_and_rows(seed):
    _, M = golden_model()
    level, items, ctx, want = kit.cached(random_rate_case, seed, 250)
    assert (want["num_sig"] == 0).any() and (want["num_sig"] > 300).any() and len(set(zip(items["w"], items["h"]))) == len(rrc.SHAPES) + len(rrc.CHROMA_ONLY)
    same_rate(chain.run_rate(M, level, items, ctx), want)


def test_choose_random():
    c = rrc.random_choose(77, 500)
    want = rrc.choose(c["tr"], c["abs_sum"], c["dist_resi"], c["zero_dist"], c["frac_bits"], c["cbf_bits"], c["prev"], c["weight"], c["scale"])
    assert (want["slot"] == -1).any() and len(set(want["slot"])) == 7 and (want["cbf"] == 0).any()
    chain.same_choose(chain.run_choose(c), want)


def long_case():
    """more items than the grid has wavefronts: 64 different small blocks, repeated"""
    level, items, ctx, want = random_rate_case(5, 64)
    reps = 600
    return level, np.tile(items, reps), ctx, {k: np.tile(v, (reps,) + (1,) * (v.ndim - 1)) for k, v in want.items()}


def test_rate_list_longer_than_the_grid():
    _, M = golden_model()
    level, items, ctx, want = kit.cached(long_case)
    assert len(items) > 4 * 8 * 304
    same_rate(chain.run_rate(M, level, items, ctx), want)


SKIPS = dict(w3=dict(w=3), w128=dict(w=128), h0=dict(h=0), h1=dict(h=1), ctx_low=dict(ctx_idx=-1), ctx_high=dict(ctx_idx=6), level_neg=dict(level_off=-16),
             luma2=dict(luma=2), dq_neg=dict(dep_quant=-1), sbh2=dict(sign_hiding=2), ts2=dict(ts_flag=2), ts_low=dict(ts_flag=-2), emt4=dict(emt_idx=4),
             emt_low=dict(emt_idx=-2), inter2=dict(emt_inter=2), thr2=dict(emt_thr=-1), reserved=dict(reserved=[0, 0, 0, 0, 0, 0, 0, 0, 1]), gate=dict())


def skip_case():
    g = rrc.golden()
    level, items, ctx = rrc.random_list(21, 3 * len(SKIPS))
    gate = np.arange(len(items), dtype=np.uint32)                           # abs sums: anything but the marker serves, 0 included
    for j, (name, change) in enumerate(SKIPS.items()):
        for field, v in change.items():
            items[3 * j + 1][field] = v
        if name == "gate":
            gate[3 * j + 1] = rrc.U32_MAX
    return level, items, ctx, gate, chain.want_rate(level, items, gate, ctx, g["est_bits"], g["next_state"])


def test_skip_markers_leave_the_rows_untouched():
    _, M = golden_model()
    level, items, ctx, gate, want = kit.cached(skip_case)
    skipped = want["frac_bits"] == rrc.U64_MAX
    assert skipped.sum() == len(SKIPS) and (want["ctx_out"][skipped] == chain.CTX_CANARY).all() and (want["num_sig"][skipped] == rrc.U32_MAX).all()
    same_rate(chain.run_rate(M, level, items, ctx, gate), want)


def chain_case(dq):
    """a short list for the pixel pass: EMT items, transform-skip items, large items, a skipped item; luma, Cb, Cr in turn"""
    bd = 10
    rng = np.random.default_rng(31 + dq)
    plane = irc.fresh_plane(rng, bd)
    shapes = [(4, 4), (8, 8), (4, 4), (16, 16), (8, 4), (16, 8), (32, 32), (4, 4), (4, 16), (64, 64), (16, 16), (8, 8)]
    specs = []
    for k, (w, h) in enumerate(shapes):
        x, y = irc.place(rng, w, h)
        small = w == 4 and h == 4 and not dq
        tr = [0, irc.TS] if small and k % 2 == 0 else [0] + list(irc.EMT) + ([irc.TS] if small else []) if k % 3 == 0 and w <= 32 else [0]
        specs.append(dict(x=x, y=y, w=w, h=h, tr=tr, qp=(22, 27, 37)[k % 3] + 6 * (bd - 8), sbh=k % 2))
    specs.append(dict(x=8, y=8, w=3, h=8))                                   # skipped by the pass: its gate skips the six rate items
    case = dqc.make(bd, plane, specs, rng) if dq else irc.make(bd, plane, specs, rng)
    luma = (np.arange(len(specs)) % 3 == 0).astype(np.int8)
    g = rrc.golden()
    ctx = np.stack([g["ctx_before"][2], g["ctx_before"][len(g["ctx_before"]) - 2]])      # a luma and a chroma row of the golden snapshots
    return case, chain.rate_items(case.items, luma, dq), ctx, chain.chain_inputs(len(specs), 5 + dq)


@pytest.mark.parametrize("dq", [0, 1])
def test_chain_behind_the_inter_residual_pass(dq):
    g, M = golden_model()
    case, ritems, ctx, extra = kit.cached(chain_case, dq)
    if dq:
        D = inter_resi_dq_chain.Device(case.bd, case.org, case.pred, case.items, case.dq, case.rates, case.cand_size, case.level_size, inter_resi_dq_chain.FILLS)
    else:
        D = inter_resi_code_chain.Device(case.bd, case.org, case.pred, case.items, case.cand_size, case.level_size, inter_resi_code_chain.FILLS)
    level, abs_sum, dist_resi, zero_dist, rate, chosen = chain.run_chain(D, M, ritems, ctx, *extra)
    want_rate, want_chosen = chain.want_chain(case.items, ritems, level, abs_sum, dist_resi, zero_dist, ctx, g["est_bits"], g["next_state"], *extra)
    served = abs_sum != rrc.U32_MAX
    assert (abs_sum[served] > 0).sum() >= 8 and (abs_sum[-1] == rrc.U32_MAX).all() and (want_rate["frac_bits"].reshape(-1, 6)[~served] == rrc.U64_MAX).all()
    assert want_chosen["slot"][-1] == -1 and (want_chosen["slot"][:-1] >= 0).all() and (want_chosen["cbf"] == 1).any()
    same_rate(rate, want_rate, ("frac_bits", "num_sig"))
    chain.same_choose(chosen, want_chosen)
