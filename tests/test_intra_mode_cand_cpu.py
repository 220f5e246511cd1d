"""vvcgpu_intra_mode_cand_batch without a device: the restatement of the pass (tests/intra_mode_cand_cases.py) against the reference's values
(tests/golden/intra_mode_cand.npz), the list logic on hand-made SATD tables -- ties, the second round's guard, the append, the three cuts --, the host
lists of the chain (tests/intra_mode_cand_chain.py) against the restatement, and the argument checks the entry makes before any device work."""
import ctypes as C

import numpy as np
import pytest

import intra_mode_cand_cases as imc
from vvcsoftware_vtm_amd import capi

ONE = 1 << 15


@pytest.mark.parametrize("bd", [8, 10])
def test_restatement_equals_golden(bd):
    g = np.load(imc.GOLDEN)
    case, flags, lam = imc.golden_case(g, bd)
    k = "bd%d_" % bd
    seen = set()
    got = imc.restate(case, flags, lam, seen=seen)
    assert np.array_equal(got["satd"], g[k + "satd"])
    assert np.array_equal(got["lists"], g[k + "lists"])
    assert got["costs"].tobytes() == g[k + "costs"].tobytes()
    assert np.array_equal(got["refs"], g[k + "refs"])
    assert {"MPM in the list", "even MPM appended", "unevaluated odd MPM appended", "shared child", "all 35 SATDs equal"} <= seen, seen
    assert {0, 1, 2} <= set(got["lists"][:, 0])


def table(default, **modes):
    t = {m: default for m in range(imc.N_MODES)}
    t.update({int(k[1:]): v for k, v in modes.items()})
    return lambda m: t[m]


def lists_of(sad_of, mpm=(0, 1, 50), num=3, bits=(0, 0, 0, 0), inter_had=imc.U64_MAX, flags=imc.USE_MPM, lam=0.0):
    satd, row, cost = imc.list_pass(sad_of, mpm, num, bits, inter_had, flags, lam)
    return satd, [int(v) for v in row], cost


def test_flat_table_order_comes_from_visiting_order_and_bits():
    """equal SATDs everywhere: strict '<' keeps the earlier visited mode ahead; with bits, the cheap MPMs come first"""
    satd, row, cost = lists_of(table(100), flags=0)
    assert row[:5] == [3, 3, 0, 1, 2] and row[5:8] == [0, 1, 2] and row[8:] == [-1] * 8
    assert cost[0] == cost[1] == cost[2] == 100.0 and (cost[3:8] == imc.INF).all() and cost[11] == imc.INF
    evaluated = [m for m in range(67) if satd[m] != imc.U64_MAX]
    assert evaluated == imc.ROUND1                                          # parents 0, 1, 2 have no children
    _, row, cost = lists_of(table(100), mpm=(40, 6, 66), bits=(ONE, 2 * ONE, 2 * ONE, 6 * ONE), flags=0, lam=0.5)
    assert row[5:8] == [40, 6, 66] and row[2:5] == [0, 1, 2]
    assert list(cost[:3]) == [100.0 + ONE * 0.5, 100.0 + 2 * ONE * 0.5, 100.0 + 2 * ONE * 0.5]


def test_second_round_and_its_guard():
    satd, row, _ = lists_of(table(500, m32=10, m34=11, m33=5, m66=12, m31=600, m35=600), flags=0)
    evaluated = [m for m in range(67) if satd[m] != imc.U64_MAX]
    assert evaluated == sorted(imc.ROUND1 + [31, 33, 35])                   # 33 once, nothing beside 66
    assert row[5:8] == [33, 32, 34] and row[2:5] == [33, 32, 34]
    # a child equal to its parent stays behind it; the parent list is the round-1 list, a child that enters brings no children of its own
    satd, row, _ = lists_of(table(500, m20=10, m21=10, m19=10, m22=400), flags=0)
    assert row[5:8] == [20, 19, 21] and satd[23] != imc.U64_MAX and satd[18] != imc.U64_MAX
    satd, row, _ = lists_of(table(500, m20=10, m21=9), num=1, flags=0)
    assert row[5:8] == [21, -1, -1] and row[0] == 1 and satd[22] == 500 and satd[23] == imc.U64_MAX


def test_mpm_append():
    t = table(500, m10=1, m12=2, m14=3, m11=400, m13=400, m9=400, m15=400)
    assert lists_of(t, mpm=(10, 12, 14))[1][5:] == [10, 12, 14] + [-1] * 8                     # all included
    assert lists_of(t, mpm=(10, 40, 14))[1][5:] == [10, 12, 14, 40] + [-1] * 7                 # an even one appended
    assert lists_of(t, mpm=(45, 1, 13))[1][5:] == [10, 12, 14, 45, 1, 13] + [-1] * 5           # 45 was never evaluated, 13 was and lost
    assert lists_of(t, mpm=(45, 1, 13), flags=0)[1][:8] == [3, 3, 10, 12, 14, 10, 12, 14]
    _, row, cost = lists_of(table(500, m2=1), mpm=(3, 4, 5), num=8)         # eight in the list, 4 among them: the longest row
    assert row[0] == 10 and row[5:16] == [2, 0, 1, 4, 6, 8, 10, 12, 3, 5, -1]
    _, row, cost = lists_of(table(500, m2=1), mpm=(3, 5, 7), num=8)
    assert row[0] == 11 and row[5:16] == [2, 0, 1, 4, 6, 8, 10, 12, 3, 5, 7]
    assert (cost[:8] != imc.INF).all() and (cost[8:11] == [1.0, 500.0, 500.0]).all() and cost[11] == imc.INF   # the appended MPMs carry no cost


def test_pbintra_cuts():
    t = table(5000, m10=100, m12=200, m14=300, m11=4000, m13=4000, m9=4000, m15=4000)
    mpm = (10, 40, 41)
    full = [10, 12, 14, 40, 41]
    assert lists_of(t, mpm=mpm, inter_had=1000)[1][:10] == [5, 3, 10, 12, 14] + full
    assert lists_of(t, mpm=mpm, inter_had=273)[1][:10] == [5, 3, 10, 12, 14] + full            # 300 > 300.3 is false
    assert lists_of(t, mpm=mpm, inter_had=272)[1][:10] == [2, 3, 10, 12, 14, 10, 12, -1, -1, -1]
    assert lists_of(t, mpm=mpm, inter_had=181)[1][:10] == [1, 3, 10, 12, 14, 10, -1, -1, -1, -1]
    assert lists_of(t, mpm=mpm, inter_had=90)[1] == [0, 3, 10, 12, 14] + [-1] * 11             # the early return
    assert lists_of(t, mpm=mpm, inter_had=0)[1][0] == 0
    assert lists_of(t, mpm=mpm, inter_had=imc.U64_MAX)[1][0] == 5
    assert list(lists_of(t, mpm=mpm, inter_had=90)[2][8:11]) == [100.0, 200.0, 300.0]


def test_cost_is_a_product_then_a_sum():
    big, lam = (1 << 40) + 12345, 1048575.984375
    _, _, cost = lists_of(table(7), bits=(big, big, big, big), lam=lam, flags=0)
    assert cost[0] == 7.0 + float(big) * lam


@pytest.mark.parametrize("bd", [8, 10])
def test_chain_host_lists_equal_the_restatement(bd):
    """the host's part of the chain (vectorised, stable sorts) on the restatement's own SATDs"""
    import intra_mode_cand_chain as chain
    case, want = imc.fresh_case(bd)
    pus, satd = case.pus, want["satd"]
    rd_c, rd_m, had_c, had_m, r2 = chain.host_round1(pus, satd[:, imc.ROUND1], 23.75)
    n = len(pus)
    rows = np.arange(n)[:, None]
    for q in range(n):                                                        # the second round's modes: the odd modes the restatement evaluated
        assert sorted(int(m) for m in r2[q] if m >= 0) == [m for m in range(3, 67, 2) if satd[q][m] != imc.U64_MAX], q
    satd2 = np.where(r2 >= 0, satd[rows, np.maximum(r2, 0)], 0).astype(np.uint64)
    lists, costs = chain.host_tail(pus, (rd_c, rd_m, had_c, had_m), r2, satd2, imc.USE_MPM, 23.75, True)
    assert np.array_equal(lists, want["lists"]) and costs.tobytes() == want["costs"].tobytes()


def entry(*a):
    return capi.lib().vvcgpu_intra_mode_cand_batch(*a)


def test_argument_checks_without_device():
    one = C.c_void_p(16)                                                      # a non-null, aligned address that is never read: every check comes first
    #     rec  flags fill refs org  pus  n  ctl  bits had  flags lambda bd  clp       satd list cost stream
    ok = [one, one, one, one, one, one, 1, one, one, one, 3, 2.0, 10, 0, 1023, one, one, one, None]
    assert entry(*(ok[:6] + [0] + ok[7:])) == 0                               # n == 0: a no-op, whatever else is passed
    assert entry(*[None if isinstance(v, C.c_void_p) else 0 if i == 6 else v for i, v in enumerate(ok)]) == 0

    def refused(changes, code=-1, word=None):
        a = list(ok)
        for i, v in changes.items():
            a[i] = v
        rc = entry(*a)
        text = capi.lib().vvcgpu_last_error().decode()
        assert rc == code and text.startswith("intra_mode_cand_batch:"), (changes, rc, text)
        if word:
            assert word in text, text
    for i in (4, 5, 7, 8, 16, 17):                                            # every required array
        refused({i: None}, word="null pointer")
    for gone in ((0,), (1,), (2,), (0, 1), (0, 2), (1, 2)):                   # rec_base, flags_base and fill: all or none
        refused({i: None for i in gone}, word="null pointer")
    refused({0: None, 1: None, 2: None, 3: None}, word="null pointer")        # neither fill nor refs_base
    refused({6: -1})
    refused({10: 4}, word="flags")
    refused({10: -1}, word="flags")
    refused({13: 5, 14: 4}, word="clip range")
    refused({14: 32768}, word="clip range")
    for lam in (-1.0, float("nan"), float("inf"), 1048576.0):
        refused({11: lam}, word="sqrt_lambda")
    refused({5: C.c_void_p(8)}, word="16-byte aligned")
    refused({2: C.c_void_p(24)}, word="16-byte aligned")
    refused({12: 12}, code=-3, word="bit depth")
    refused({12: 7}, code=-3, word="bit depth")
