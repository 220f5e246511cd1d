"""GPU parity on the inputs of tests/cases.py::deblock_census_cases: vvcgpu_deblock bit-equal to the restatement on all three planes where every filter decision
sits on its threshold (tests/test_deblock_census_cpu.py counts the events these inputs reach), through the block form, the tile form and the luma-only call."""
import ctypes as C

import numpy as np
import pytest
import torch

import cases
from oraclelib import oracle, p

pytestmark = pytest.mark.gpu

CASES = cases.deblock_census_cases()
IDS = [c["name"] for c in CASES]
SPARE = 12345                      # what the two spare columns of a tile-form row hold
_want = {}


def dev(a):
    return torch.from_numpy(a).cuda()


def want(i):
    """the restatement's planes of case i: computed once, shared by the three forms, never written"""
    if i not in _want:
        c = CASES[i]
        cfg = cases.deblock_cfg_struct(c["cfg"])
        Y, Cb, Cr = c["Y"].copy(), c["Cb"].copy(), c["Cr"].copy()
        oracle().orc_deblock(p(Y), c["w"], p(Cb), p(Cr), c["w"] // 2, c["w"], c["h"], p(c["ev"]), p(c["eh"]), p(c["qpl"]), p(c["qpc"]), C.byref(cfg))
        for a in (Y, Cb, Cr):
            a.setflags(write=False)
        _want[i] = (Y, Cb, Cr)
    return _want[i]


def check(got, i):
    for g, w_, name in zip(got, want(i), "Y Cb Cr".split()):
        g = g.cpu().numpy()
        assert np.array_equal(g, w_), "%s %s: %d samples differ, first at %s" % (IDS[i], name, int((g != w_).sum()), np.argwhere(g != w_)[0])


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_block_form(i):
    from vvcsoftware_vtm_amd import ops
    c = CASES[i]
    d = [dev(c[k]) for k in ("Y", "Cb", "Cr")]
    ops.deblock(d[0], d[1], d[2], dev(c["ev"]), dev(c["eh"]), dev(c["qpl"]), dev(c["qpc"]), cases.deblock_cfg_struct(c["cfg"]))
    check(d, i)


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_tile_form(i):
    """rows of w + 2 samples are no whole 8-byte words: the LDS tile form; the spare columns stay as they were"""
    from vvcsoftware_vtm_amd import ops
    c = CASES[i]
    src = [c[k] for k in ("Y", "Cb", "Cr")]
    big = [torch.full((a.shape[0], a.shape[1] + 2), SPARE, dtype=torch.int16, device="cuda") for a in src]
    views = [b[:, :a.shape[1]] for a, b in zip(src, big)]
    for v, a in zip(views, src):
        v.copy_(dev(a))
    ops.deblock(views[0], views[1], views[2], dev(c["ev"]), dev(c["eh"]), dev(c["qpl"]), dev(c["qpc"]), cases.deblock_cfg_struct(c["cfg"]))
    check(views, i)
    assert all(bool((b[:, -2:] == SPARE).all()) for b in big)


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_luma_only(i):
    """no chroma planes and no chroma QP map: luma as in the full call"""
    from vvcsoftware_vtm_amd import ops
    c = CASES[i]
    dY = dev(c["Y"])
    ops.deblock(dY, None, None, dev(c["ev"]), dev(c["eh"]), dev(c["qpl"]), None, cases.deblock_cfg_struct(c["cfg"]))
    check([dY], i)

