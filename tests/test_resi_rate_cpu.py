"""vvcgpu_resi_rate_batch and vvcgpu_inter_resi_choose_batch without a device: the restatement (tests/resi_rate_cases.py) reproduces every value the
compiled reference gave (tests/golden/resi_rate.npz), the golden file is integer data under the cap, the mirror of struct vvcgpu_resi_rate_item and the
VVCGPU_RESI_RATE_* constants are the header's, and both entries check their arguments before any device work."""
import ctypes as C
import os
import re
import shlex
import subprocess

import numpy as np

import rd_pass_kit as kit
import resi_rate_cases as rrc
from vvcsoftware_vtm_amd import abi, capi


def test_restatement_reproduces_the_golden_rates():
    g = rrc.golden()
    items = np.ascontiguousarray(g["items"]).view(abi.RESI_RATE_ITEM).reshape(-1)
    assert len(items) > 800 and {(int(w), int(h)) for w, h in zip(items["w"], items["h"])} == set(rrc.SHAPES + rrc.CHROMA_ONLY)
    assert {(int(a), int(b)) for a, b in zip(items["dep_quant"], items["sign_hiding"])} == set(rrc.FLAGS)
    want = rrc.restate(g["level"], items, None, g["ctx_before"], g["est_bits"], g["next_state"])
    kit.check_restatement(want, dict(frac_bits=g["bits"], num_sig=g["num_sig"], ctx_out=g["ctx_after"]), "resi_rate")
    assert (g["num_sig"] == 0).any() and (g["ctx_before"][:, :abi.RESI_RATE_CTX_USED].min() <= 1) and g["ctx_before"].max() >= 124
    assert not g["ctx_before"][:, abi.RESI_RATE_CTX_USED:].any() and np.abs(g["level"]).max() == 32767


def test_restatement_reproduces_the_golden_compare():
    g = rrc.golden()
    want = rrc.choose(g["choose_tr"], g["choose_abs_sum"], g["choose_dist_resi"], g["choose_zero_dist"], g["choose_frac_bits"], g["choose_cbf_bits"],
                      g["choose_prev"], g["choose_weight"].view(np.float64), float(g["choose_scale"].view(np.float64)[0]))
    for k, v in want.items():
        assert v.tobytes() == g["choose_out_" + k].tobytes(), k
    assert g["choose_out_slot"][0] == 1 and (g["choose_out_slot"] == -1).any()          # the transform-skip tie; skipped items


def test_golden_file():
    kit.check_golden_file(rrc.GOLDEN)


def test_model_tables_are_a_probability_model():
    g = rrc.golden()
    est, nxt = g["est_bits"], g["next_state"]
    assert est.shape == (128,) and nxt.shape == (256,) and nxt.max() < 128
    assert est.min() > 0 and est.max() < 1 << 20                                       # a bin costs less than 32 bits: the kernel's sums cannot wrap


def test_item_mirror_matches_the_header(tmp_path):
    """the C compiler's sizeof / offsetof of struct vvcgpu_resi_rate_item == abi.RESI_RATE_ITEM, field by field; the constants of the row"""
    names = abi.RESI_RATE_ITEM.names
    src = tmp_path / "layout.c"
    src.write_text("#include <stddef.h>\n#include <stdio.h>\n#include \"vvcgpu.h\"\nint main(void)\n{\n"
                   "  printf(\"%zu\\n\", sizeof(struct vvcgpu_resi_rate_item));\n"
                   + "".join('  printf("%%s %%zu %%zu\\n", "%s", offsetof(struct vvcgpu_resi_rate_item, %s), sizeof(((struct vvcgpu_resi_rate_item*)0)->%s));\n'
                             % (f, f, f) for f in names) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    cc = shlex.split(os.environ.get("CC", "cc"))
    r = subprocess.run(cc + ["-I", os.path.dirname(capi.HEADER), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = subprocess.check_output([str(exe)], text=True).splitlines()
    assert int(lines[0]) == abi.RESI_RATE_ITEM.itemsize == 32
    for line in lines[1:]:
        f, off, size = line.split()
        dt, at = abi.RESI_RATE_ITEM.fields[f][:2]
        assert (int(off), int(size)) == (at, dt.itemsize), f
    hdr = " ".join(open(capi.HEADER).read().split())
    for name in ("CTX_BYTES", "CTX_USED", "LAST_X", "LAST_Y", "SIG_GROUP", "SIG", "PAR", "GT2", "GT1", "TS", "EMT"):
        assert int(re.search(r"#define VVCGPU_RESI_RATE_%s (\d+) " % name, hdr).group(1)) == getattr(abi, "RESI_RATE_" + name), name
    regions = [(abi.RESI_RATE_LAST_X, 25), (abi.RESI_RATE_LAST_Y, 25), (abi.RESI_RATE_SIG_GROUP, 2), (abi.RESI_RATE_SIG, 60), (abi.RESI_RATE_PAR, 21),
               (abi.RESI_RATE_GT2, 21), (abi.RESI_RATE_GT1, 21), (abi.RESI_RATE_TS, 1), (abi.RESI_RATE_EMT, 4)]
    assert [at for at, _ in regions] == list(np.cumsum([0] + [size for _, size in regions[:-1]])) and sum(s for _, s in regions) == abi.RESI_RATE_CTX_USED
    assert "typedef struct vvcgpu_resi_rate_item" not in hdr                           # a plain tagged struct: tests/test_abi.py's census stays as it is


def test_prototypes():
    protos = capi.prototypes()
    assert protos["vvcgpu_resi_rate_batch"] == (C.c_int, (C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int) + (C.c_void_p,) * 6)
    assert protos["vvcgpu_inter_resi_choose_batch"] == (C.c_int, (C.c_void_p, C.c_int) + (C.c_void_p,) * 7 + (C.c_double,) + (C.c_void_p,) * 7)


def test_entries_check_their_arguments_without_a_device():
    if not os.path.exists(capi.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = capi.lib()
    x = C.c_void_p(256)                                                      # never dereferenced: the checks come before any device work

    def rate(**kw):
        a = dict(level=x, items=x, n=3, gate=None, ctx=x, n_ctx=2, est=x, nxt=x, frac=x, nsig=x, ctx_out=None)
        a.update(kw)
        return lib.vvcgpu_resi_rate_batch(a["level"], a["items"], a["n"], a["gate"], a["ctx"], a["n_ctx"], a["est"], a["nxt"], a["frac"], a["nsig"],
                                          a["ctx_out"], None)

    def choose(**kw):
        a = dict(items=x, n=3, abs_sum=x, dist_resi=x, zero_dist=x, frac=x, cbf_bits=x, prev=x, weight=x, slot=x, cbf=x, abs_out=x, dist=x, bits=x, cost=x)
        a.update(kw)
        return lib.vvcgpu_inter_resi_choose_batch(a["items"], a["n"], a["abs_sum"], a["dist_resi"], a["zero_dist"], a["frac"], a["cbf_bits"], a["prev"],
                                                  a["weight"], C.c_double(100.0), a["slot"], a["cbf"], a["abs_out"], a["dist"], a["bits"], a["cost"], None)

    bad_rate = [dict(level=None), dict(items=None), dict(ctx=None), dict(est=None), dict(nxt=None), dict(frac=None), dict(nsig=None), dict(n=-1),
                dict(n_ctx=0), dict(n_ctx=-2), dict(items=C.c_void_p(260))]
    for kw in bad_rate:
        assert rate(**kw) == -1, kw
        assert b"resi_rate_batch" in lib.vvcgpu_last_error(), kw
    bad_choose = [{k: None} for k in ("items", "abs_sum", "dist_resi", "zero_dist", "frac", "cbf_bits", "prev", "weight", "slot", "cbf", "abs_out", "dist",
                                      "bits", "cost")] + [dict(n=-1), dict(items=C.c_void_p(264))]
    for kw in bad_choose:
        assert choose(**kw) == -1, kw
        assert b"inter_resi_choose_batch" in lib.vvcgpu_last_error(), kw
    # n == 0 is a no-op, whatever else is given
    assert rate(n=0) == 0 and rate(n=0, level=None, items=None, ctx=None, n_ctx=0) == 0
    assert choose(n=0) == 0 and choose(n=0, items=None, prev=None) == 0
