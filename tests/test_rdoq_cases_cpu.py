"""What the lists of tests/rdoq_cases.py reach, counted by the oracle alone (orc_rdoq_events): tests/test_gpu_quantisers.py compares the device with the
oracle on these lists, and that comparison only means something for a branch that the lists take.  No GPU here."""
import functools

import numpy as np
import pytest

import rdoq_cases as rc
from rdoq_cases import EV

# every outcome of the sign-hiding search but the forced step down at the level cap (cap_case's: a level of 32767 needs bit depth 10 and a large TU), the
# three Rice parameters and the escape code under each
SBH_OUTCOMES = ("sbh_new", "sbh_new_before_first", "sbh_up", "sbh_down", "sbh_down_to_zero", "sbh_bonus_chosen", "sbh_refused_by_sign")
RICE = ("rice0", "rice1", "rice2", "escape_rice0", "escape_rice1", "escape_rice2")
# a TU of one or two groups has no group below its last one except group 0, which takes none of these branches
GROUPS = ("cg_empty", "cg_zeroed", "cg_nnz_before_pos0_zero", "last_truncated", "last_kept")


@functools.lru_cache(maxsize=None)
def cached(name, *args):
    return getattr(rc, name)(*args)


def test_event_read_out_counts_and_clears():
    """one 8x8 TU with a single large level at the end of the scan: one kept last position, all 64 positions in range (the five that have the level in their
    template take Rice parameter 2), two empty groups between the last group and group 0, no sign hiding; a second read returns zeros"""
    coef = np.zeros(64, np.int32)
    coef[63] = 20000
    c = rc.make(rc.RDOQ, 10, [rc.spec(8, 8, coef, 30, 30.0, 1, 1, 0)])
    e = c.events[0]
    assert c.want_sum[0] > 0 and e[EV["last_kept"]] == 1 and e[EV["rice0"]] == 59 and e[EV["rice2"]] == 5 and e[EV["last_truncated"]] == e[EV["last_zero"]] == 0
    assert e[EV["cg_empty"]] == 2 and e[EV["sbh_new"]] == e[EV["sbh_up"]] == e[EV["sbh_down"]] == 0
    assert not rc.read_events().any()


@pytest.mark.parametrize("bd", [8, 10])
def test_shapes_case_reaches_every_branch_on_every_shape(bd):
    c = cached("shapes_case", bd)
    d = c.descs
    assert {(int(w), int(h)) for w, h in zip(d["w"], d["h"])} == set(rc.all_shapes())
    for (w, h) in rc.all_shapes():
        sel = (d["w"] == w) & (d["h"] == h)
        assert sel.sum() >= 12
        assert set(d["luma"][sel]) == {0, 1} and set(d["sign_hiding"][sel]) == {0, 1} and {0, rc.max_qp(bd)} <= set(d["qp"][sel])
        e = c.cell_events(w, h)
        missing = [n for n in SBH_OUTCOMES + RICE + (GROUPS if w * h >= 64 else ()) if e[EV[n]] < 1]
        assert not missing, (w, h, missing)
    assert c.events[:, EV["last_zero"]].sum() >= 1 and c.events[:, EV["last_walk_ended_gt1"]].sum() >= 1
    # the layout: offsets in multiples of 16, the two offsets differ for part of the TUs, the tables come from all over the file
    assert not (d["coeff_off"] % 16).any() and not (d["level_off"] % 16).any()
    assert 0 < (d["coeff_off"] != d["level_off"]).sum() < len(d) and len(set(d["rates_idx"])) > 100 and len(c.rates) == 150


def test_cap_case_reaches_the_cap_on_each_shape_and_the_forced_step_down():
    c = cached("cap_case")
    assert c.bd == 10 and len(rc.CAP_SHAPES) == 10 and (c.descs["sign_hiding"] == 1).all() and set(c.descs["qp"]) == {0, 1, 2}
    for (w, h) in rc.CAP_SHAPES:
        assert c.cell_events(w, h)[EV["level_capped"]] >= 1, (w, h)
    assert c.events[:, EV["sbh_forced_at_cap"]].sum() >= 8
    assert (np.abs(c.want_level[c.want_level != rc.LEVEL_CANARY]) == 32767).any() and (np.abs(c.want_level[c.want_level != rc.LEVEL_CANARY]) == 32766).any()


@pytest.mark.parametrize("bd", [8, 10])
def test_margin_case_sits_on_the_all_zero_decision(bd):
    c = cached("margin_case", bd)
    d = c.descs
    assert [(int(w), int(h)) for w, h in zip(d["w"][0::2], d["h"][0::2])] == rc.all_shapes()
    assert (d["lambda"][1::2] == np.nextafter(d["lambda"][0::2], np.inf)).all()               # neighbouring doubles
    assert (c.want_sum[0::2] > 0).all() and (c.want_sum[1::2] == 0).all()
    assert (c.events[1::2, EV["last_zero"]] == 1).all() and (c.events[0::2, EV["last_zero"]] == 0).all()
    # behind the last level of the coded TU lie coefficients that quantise to nothing but cost something uncoded
    for i in range(0, len(d), 2):
        co, n = int(d["coeff_off"][i]), int(d["w"][i]) * int(d["h"][i])
        assert np.count_nonzero(c.coef[co:co + n]) > np.count_nonzero(c.tu_level(i))


@pytest.mark.parametrize("n", rc.PACKING_COUNTS)
@pytest.mark.parametrize("kind", [rc.RDOQ, rc.DEPQUANT])
def test_packing_case_has_one_all_zero_tu_per_team_slot(kind, n):
    c = cached("packing_case", n, kind)
    d = c.descs
    assert len(d) == n
    zero = [i for i in range(n) if not c.coef[int(d["coeff_off"][i]):int(d["coeff_off"][i]) + int(d["w"][i]) * int(d["h"][i])].any()]
    assert len(zero) == len({i % 4 for i in zero}) == (4 if n >= 15 else 1 if n >= 2 else 0)  # one per slot where the batch is long enough, TU 0 live
    assert len({i // 4 for i in zero}) == len(zero)                                         # each beside live teams
    for i in zero:
        assert c.want_sum[i] == 0 and not c.tu_level(i).any()
    assert (c.want_sum > 0).sum() >= (n - len(zero) + 1) // 2
    if n >= 4:                                                                              # a 256-group team beside one-group teams in wavefront 0
        assert (int(d["w"][0]), int(d["h"][0])) == (64, 64) and (int(d["w"][1]), int(d["h"][1])) == (4, 4)


@pytest.mark.parametrize("kind", [rc.RDOQ, rc.DEPQUANT])
def test_workspace_cases_share_offsets_under_other_shapes(kind):
    c1, c2 = cached("workspace_cases", kind)
    shapes = lambda c: [(int(w), int(h)) for w, h in zip(c.descs["w"], c.descs["h"])]
    assert shapes(c1) == [(64, 64), (64, 16), (16, 64)] and shapes(c2) == [(16, 16), (32, 64), (8, 32), (4, 4)]
    assert c1.total == c2.total and list(c2.descs["coeff_off"][:2]) == list(c1.descs["coeff_off"][:2])
    assert (c1.want_sum > 0).all() and (c2.want_sum > 0).sum() >= 3


@pytest.mark.parametrize("bd", [8, 10])
def test_depquant_shapes_case_covers_every_shape(bd):
    c = cached("shapes_case", bd, rc.DEPQUANT)
    d = c.descs
    for (w, h) in rc.all_shapes():
        sel = (d["w"] == w) & (d["h"] == h)
        assert sel.sum() >= 12 and (c.want_sum[sel] > 0).sum() >= 6 and {0, rc.max_qp(bd)} <= set(d["qp"][sel])
    assert len(set(d["rates_idx"])) > 80 and len(c.rates) == 100
    levels = c.want_level[c.want_level != rc.LEVEL_CANARY]
    assert np.abs(levels).max() > 255                                                       # beyond the byte the level histories keep
