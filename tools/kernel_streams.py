#!/usr/bin/env python3
"""Instruction streams and resource notes of the device functions of two trees, side by side: the check of a refactor that must leave kernels as they are.

Each source is compiled in both trees with the flags of vvcsoftware_vtm_amd/build.py plus --cuda-device-only -S.  Per function (kernels and the
__noinline__ bodies they call) the instruction lines between its label and its .Lfunc_end are compared: mnemonic and operands only; comments,
directives and labels are dropped, block labels lose their function number, and symbol names are replaced by the readable name.  Kernels also show
what their metadata notes say: VGPR, AGPR, spilled VGPR, static LDS, scratch.

usage: python tools/kernel_streams.py PARENT_TREE THIS_TREE source [source ..] [--same here=parent ..] [--all]
  source      a file name under vvcsoftware_vtm_amd/csrc, with or without .hip
              HERE=PARENT where the source has another name in the parent, e.g. after a split: saostats=stats alfstats=stats
  --same      a function of this tree that is to be compared with a function of another name in the parent (readable names, as the table prints them)
  --all       list the identical non-kernel functions too (default: their number)
"""
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-fno-fast-math", "-ffp-contract=off"]   # build.py's, the include paths follow per tree


def readable(sym):
    """_ZN12_GLOBAL__N_123intra_tu_dq_back_kernelE.. -> intra_tu_dq_back_kernel; integer and bool template arguments are kept, and so is the class of a
    static member: _ZN12_GLOBAL__N_17ItqPassILb0EE4backE.. -> ItqPass<0>::back"""
    m = re.match(r"_ZN12_GLOBAL__N_1(?=\d)", sym) or re.match(r"_Z(?=\d)", sym)
    if not m:
        return sym
    pos, parts = m.end(), []
    while True:
        n = re.match(r"\d+", sym[pos:])
        if not n:
            break
        pos += n.end()
        name = sym[pos:pos + int(n.group(0))]
        pos += len(name)
        args = re.match(r"I((?:L[ib]\d+E)+)E", sym[pos:])
        if args:
            name += "<%s>" % ", ".join(re.findall(r"L[ib](\d+)E", args.group(1)))
            pos += args.end()
        parts.append(name)
        if not sym.startswith("_ZN"):
            break
    return "::".join(parts)


def compile_s(tree, src, out):
    csrc = os.path.join(tree, "vvcsoftware_vtm_amd", "csrc")
    cmd = [HIPCC] + FLAGS + ["-I" + os.path.join(tree, "include"), "-I" + csrc, "--cuda-device-only", "-S", os.path.join(csrc, src + ".hip"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("hipcc failed for %s in %s:\n%s" % (src, tree, r.stderr))
    return out


def parse(path, rename):
    """-> {readable name: (instruction list, notes or None)}"""
    funcs, notes = {}, {}
    cur, body = None, None
    sym_re = re.compile(r"_Z\w+")
    txt = open(path).read()
    is_func = set(re.findall(r"\.type\s+(\w+),@function", txt))
    for ln in txt.splitlines():
        m = re.match(r"(\w+):\s*(;.*)?$", ln)
        if m and cur is None and m.group(1) in is_func:
            cur, body = m.group(1), []
            continue
        if cur is None:
            continue
        if ln.startswith(".Lfunc_end"):
            name = readable(cur)
            funcs[rename.get(name, name)] = body
            cur = None
            continue
        s = ln.split(";")[0].strip()
        if not s or s.startswith(".") or s.endswith(":"):
            continue
        s = re.sub(r"\.LBB\d+_(\d+)", r".LBB_\1", s)
        s = sym_re.sub(lambda k: rename.get(readable(k.group(0)), readable(k.group(0))), s)
        body.append(" ".join(s.split()))
    rec = {}
    for ln in txt[txt.find(".amdgpu_metadata"):].splitlines():
        m = re.match(r"\s*-?\s*\.(\w+):\s*(.*)", ln)
        if not m:
            continue
        k, v = m.group(1), m.group(2).strip()
        if k == "agpr_count" and rec.get("name"):
            notes[readable(rec["name"])] = rec
            rec = {}
        rec[k] = v
    if rec.get("name"):
        notes[readable(rec["name"])] = rec
    return {n: (b, notes.get(n) or notes.get({v: k for k, v in rename.items()}.get(n, n))) for n, b in funcs.items()}


def main():
    argv = sys.argv[1:]
    same, show_all, pos = {}, False, []
    while argv:
        a = argv.pop(0)
        if a == "--same":
            here, parent = argv.pop(0).split("=")
            same[parent] = here
        elif a == "--all":
            show_all = True
        else:
            pos.append(a)
    if len(pos) < 3:
        sys.exit(__doc__)
    parent, here = os.path.abspath(pos[0]), os.path.abspath(pos[1])
    srcs = []                                                              # (here, parent)
    for a in pos[2:]:
        sh, _, sp = a.partition("=")
        srcs.append(tuple(s[:-4] if s.endswith(".hip") else s for s in (sh, sp or sh)))
    with tempfile.TemporaryDirectory() as tmp:
        with ThreadPoolExecutor(max_workers=8) as ex:
            done = {}                                                      # a parent source that several sources of this tree came from is compiled once

            def asm(tree, tag, s):
                if (tag, s) not in done:
                    done[tag, s] = ex.submit(compile_s, tree, s, os.path.join(tmp, tag + s + ".s"))
                return done[tag, s]

            jobs = [(asm(parent, "p_", sp), asm(here, "h_", sh)) for sh, sp in srcs]
            A, B = {}, {}
            for (s, _), (_, h) in zip(srcs, jobs):                         # a kernel by its name alone (it may move), a called body by source and name
                B.update({n if f[1] else s + ": " + n: f for n, f in parse(h.result(), {}).items()})
            for sp in dict.fromkeys(sp for _, sp in srcs):                 # the parent's under this tree's names: a called body under the source of
                heirs = [sh for sh, p in srcs if p == sp]                  # this tree that has it now, or the first that came from its source
                for n, f in parse(done["p_", sp].result(), same).items():
                    A[n if f[1] else next((sh for sh in heirs if sh + ": " + n in B), heirs[0]) + ": " + n] = f
    key = lambda r: "/".join(r.get(k, "?") for k in ("vgpr_count", "agpr_count", "vgpr_spill_count", "group_segment_fixed_size", "private_segment_fixed_size"))
    print("%-44s %13s  %-9s  %s" % ("function", "parent / here", "stream", "VGPR/AGPR/spilled/LDS/scratch   parent -> here"))
    quiet = 0
    for n in sorted(set(A) | set(B), key=lambda n: (not ((A.get(n) or B.get(n))[1]), n)):
        a, b = A.get(n), B.get(n)
        if a is None or b is None:
            print("%-44s %13s  %-9s" % (n[:44], "%s / %s" % (len(a[0]) if a else "-", len(b[0]) if b else "-"), "parent only" if a else "here only"))
            continue
        ident = a[0] == b[0]
        if ident and not a[1] and not show_all:
            quiet += 1
            continue
        res = "%s -> %s" % (key(a[1]), key(b[1])) if a[1] and b[1] else ""
        print("%-44s %13s  %-9s  %s" % (n[:44], "%d / %d" % (len(a[0]), len(b[0])), "identical" if ident else "differs", res))
    if quiet:
        print("and %d functions that are not kernels, all identical" % quiet)


if __name__ == "__main__":
    main()
