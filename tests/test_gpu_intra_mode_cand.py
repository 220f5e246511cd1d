"""vvcgpu_intra_mode_cand_batch on the device against the reference's values (tests/golden/intra_mode_cand.npz) and against the restatement of the pass
(tests/intra_mode_cand_cases.py) on a fresh seeded PU list: with and without the gathering, the optional outputs and inputs, the two flags, a narrowed
clip range, short lists, the contract's sentinel rows, two streams, and -- as a supplement -- the chain of the existing entries
(tests/intra_mode_cand_chain.py).  Every comparison is bit for bit."""
import functools

import numpy as np
import pytest
import torch

import intra_mode_cand_cases as imc
import intra_mode_cand_chain as chain
import pu_search_kit as kit
from vvcsoftware_vtm_amd import ops

pytestmark = pytest.mark.gpu

LAM = 23.75


def same(got, want, satd=True, refs=True):
    assert np.array_equal(got["lists"], want["lists"])
    assert got["costs"].tobytes() == want["costs"].tobytes()
    if satd:
        assert np.array_equal(got["satd"], want["satd"])
    if refs:
        assert np.array_equal(got["refs"], want["refs"])


@functools.lru_cache(maxsize=None)
def fresh(bd):
    case, want = imc.fresh_case(bd, sqrt_lambda=LAM)
    return case, want, chain.Device(case)


def run(D, flags=imc.USE_MPM, lam=LAM, **kw):
    refs = D.fresh_refs()
    return chain.download(chain.run_entry(D, flags, lam, refs, **kw), refs)


@pytest.mark.parametrize("bd", [8, 10])
def test_against_golden(bd):
    g = np.load(imc.GOLDEN)
    case, flags, lam = imc.golden_case(g, bd)
    k = "bd%d_" % bd
    got = run(chain.Device(case), flags, lam)
    assert np.array_equal(got["satd"], g[k + "satd"])
    assert np.array_equal(got["lists"], g[k + "lists"])
    assert got["costs"].tobytes() == g[k + "costs"].tobytes()
    assert np.array_equal(got["refs"], g[k + "refs"])


@pytest.mark.parametrize("bd", [8, 10])
def test_against_restatement(bd):
    """the fresh list, gathering inside the call: lists, costs, SATDs, and the written references equal vvcgpu_intra_fill_refs_batch's"""
    case, want, D = fresh(bd)
    got = run(D)
    same(got, want)
    refs = D.fresh_refs()
    ops.intra_fill_refs_batch(D.rec, D.avail, refs, D.fill, D.n, bd)
    torch.cuda.synchronize()
    assert got["refs"].tobytes() == refs.cpu().numpy().tobytes()


def test_references_handed_over():
    """fill == NULL: refs_base holds the references and stays as it is"""
    case, want, D = fresh(10)
    refs = torch.from_numpy(want["refs"]).cuda()
    got = chain.download(chain.run_entry(D, imc.USE_MPM, LAM, refs, fill=False), refs)
    same(got, want)


def test_optional_arrays():
    case, want, D = fresh(10)
    same(run(D, want_satd=False), want, satd=False)
    got = chain.download(chain.run_entry(D, imc.USE_MPM, LAM, None))        # gathering without a refs_base to write to
    same(got, want, refs=False)
    ungated = imc.restate(case, imc.USE_MPM, LAM, use_inter_had=False)
    assert not np.array_equal(ungated["lists"], want["lists"])
    same(run(D, gate="off"), ungated)
    same(run(D, gate="ones"), ungated)


@pytest.mark.parametrize("flags", [0, imc.NO_SMOOTHING, imc.USE_MPM | imc.NO_SMOOTHING])
def test_flags(flags):
    case, _, D = fresh(8)
    same(run(D, flags), imc.restate(case, flags, LAM))


def test_clip_range_is_the_callers():
    case, _, D = fresh(10)
    clp = (64, 700)
    same(run(D, clp=clp), imc.restate(case, imc.USE_MPM, LAM, clp))


@pytest.mark.parametrize("n", [1, 3, 5])
def test_partial_groups_of_wavefront_owners(n):
    case, want, _ = fresh(10)
    small = [q for q, u in enumerate(case.pus) if int(u["w"]) * int(u["h"]) <= 1024][7:7 + n]
    sub = imc.Case(case.rec, case.org, case.pus[small].copy(), case.avail, 10)
    sub.refs_size = case.refs_size
    got = run(chain.Device(sub))
    for i, q in enumerate(small):
        assert np.array_equal(got["lists"][i], want["lists"][q]) and got["costs"][i].tobytes() == want["costs"][q].tobytes()
        assert np.array_equal(got["satd"][i], want["satd"][q])


def test_entry_ends_where_the_chain_ends():
    case, want, D = fresh(8)
    same(run(D), chain.run_chain(D, imc.USE_MPM, LAM))


def test_contract_sentinels():
    """PUs outside the contract between good ones: the bad ones carry the sentinel rows and write no reference, the good ones keep their results"""
    case, want, _ = fresh(10)
    pick = list(range(0, 60)) + list(range(len(case.pus) - 12, len(case.pus)))
    sub = imc.Case(case.rec, case.org, case.pus[pick].copy(), case.avail, 10)
    sub.refs_size = case.refs_size
    D = chain.Device(sub)
    pus, fill, ctl = D.pus_host.copy(), D.fill_host.copy(), sub.ctl()
    bad = {}
    pus[3]["w"] = 128; fill[3]["w"] = 128; bad[3] = "side 128"
    pus[8]["h"] = 12; fill[8]["h"] = 12; bad[8] = "side 12"
    pus[13]["w"] = 0; bad[13] = "side 0"
    pus[14]["h"] = 2; fill[14]["h"] = 2; bad[14] = "side 2"
    fill[20]["w"] = int(fill[20]["w"]) ^ 12; bad[20] = "fill.w != pus.w"
    fill[24]["h"] = 2 * int(fill[24]["h"]); bad[24] = "fill.h != pus.h"
    fill[31]["ref_off"] += 1; bad[31] = "fill.ref_off != pus.ref_off"
    ctl[36][0] = 67; bad[36] = "MPM 67"
    ctl[41][2] = -1; bad[41] = "MPM -1"
    ctl[47][3] = 0; bad[47] = "numModesForFullRD 0"
    ctl[52][3] = 9; bad[52] = "numModesForFullRD 9"
    big = [i for i in range(len(pick)) if i not in bad and int(pus[i]["w"]) * int(pus[i]["h"]) > 1024]
    assert len(big) >= 4                                                      # workgroup owners' PUs: two bad ones, the others stay good
    ctl[big[0]][1] = 100; bad[big[0]] = "MPM 100 (a workgroup owner's PU)"
    fill[big[-1]]["ref_off"] -= 2; bad[big[-1]] = "fill.ref_off != pus.ref_off (a workgroup owner's PU)"
    D.pus, D.fill, D.ctl = ops.struct_to_device(pus), ops.struct_to_device(fill), kit.dev(ctl)
    got = run(D)
    guard = D.fresh_refs().cpu().numpy()
    for i, q in enumerate(pick):
        if i in bad:
            assert (got["lists"][i] == -1).all() and (got["costs"][i] == imc.INF).all() and (got["satd"][i] == imc.U64_MAX).all(), (i, bad[i])
        else:
            assert np.array_equal(got["lists"][i], want["lists"][q]) and got["costs"][i].tobytes() == want["costs"][q].tobytes(), i
            assert np.array_equal(got["satd"][i], want["satd"][q]), i
    expect = guard.copy()
    for i, q in enumerate(pick):
        if i not in bad:
            u = case.pus[q]
            a, b = int(u["ref_off"]), int(u["ref_off"]) + sum(imc.ref_lengths(int(u["w"]), int(u["h"]))) + 1
            expect[a:b] = want["refs"][a:b]
    assert np.array_equal(got["refs"], expect)


def test_two_streams():
    case, want, D = fresh(10)

    def decode(satd, lists, costs):
        return (np.concatenate([satd.cpu().numpy().view(np.uint64).reshape(-1), costs.cpu().numpy().view(np.uint64).reshape(-1)]), lists.cpu().numpy())
    kit.two_streams(lambda: chain.run_entry(D, imc.USE_MPM, LAM, D.fresh_refs()), decode,
                    (np.concatenate([want["satd"].reshape(-1), want["costs"].view(np.uint64).reshape(-1)]), want["lists"]))
