#!/usr/bin/env python3
"""Vector / matrix / LDS / scalar instruction counts per basic block of one kernel in a gfx950 assembly listing (no GPU needed):
  hipcc -S --cuda-device-only <build.FLAGS> vvcsoftware_vtm_amd/csrc/fracsearch.hip -o f.s
  python tools/isa_blocks.py f.s 'frac16m_kernelILi4ELi16' [min instructions per block listed]
A block runs from one label (or fallen-into basic block, "%bb.N") to the next; its last branch is printed, so that the loop of a kernel and its
common path can be read off (a block that branches back to an earlier label closes a loop).  The counts are of the ISA, not of time."""
import re
import sys


def main():
    path, flt = sys.argv[1], sys.argv[2]
    least = int(sys.argv[3]) if len(sys.argv) > 3 else 0
    inside = False
    blocks = []                                              # [label, {class: count}, last branch]
    for ln in open(path):
        s = ln.strip()
        m = re.match(r"^([A-Za-z_.$][\w.$]*):", s)
        if m and not s.startswith(".L") and not s.startswith(";"):
            if inside:
                break                                        # the next symbol: the kernel is over
            inside = flt in m.group(1)
            if inside:
                blocks.append([m.group(1)[:40], {}, ""])
            continue
        if not inside:
            continue
        if s.startswith(".Lfunc_end"):
            break
        if m:
            blocks.append([m.group(1), {}, ""])
            continue
        mb = re.match(r"^; (%bb\.\d+):", s)                  # a basic block that is only fallen into has no label, just this comment
        if mb:
            blocks.append([mb.group(1), {}, ""])
            continue
        if not s or s.startswith((";", ".")):
            continue
        op = s.split()[0]
        cls = ("mfma" if op.startswith("v_mfma") else "valu" if op.startswith("v_") else "lds" if op.startswith("ds_") else
               "vmem" if op.startswith(("global_", "buffer_", "flat_", "scratch_")) else "salu" if op.startswith("s_") else "other")
        c = blocks[-1][1]
        c[cls] = c.get(cls, 0) + 1
        if op.startswith(("s_cbranch", "s_branch", "s_endpgm", "s_setpc", "s_swappc")):
            blocks[-1][2] = s.split(";")[0].strip()
    tot = {}
    print("%-44s %5s %5s %5s %5s %5s  %s" % ("block", "valu", "mfma", "lds", "vmem", "salu", "ends with"))
    for lab, c, br in blocks:
        for k, v in c.items():
            tot[k] = tot.get(k, 0) + v
        if sum(c.values()) >= least:
            print("%-44s %5d %5d %5d %5d %5d  %s" % (lab, c.get("valu", 0), c.get("mfma", 0), c.get("lds", 0), c.get("vmem", 0), c.get("salu", 0), br))
    print("%-44s %5d %5d %5d %5d %5d" % ("whole kernel", tot.get("valu", 0), tot.get("mfma", 0), tot.get("lds", 0), tot.get("vmem", 0), tot.get("salu", 0)))


if __name__ == "__main__":
    main()
