#!/usr/bin/env python3
"""Phase stamps of me_hier_kernel INSIDE the 4K picture's workload (GPU box; a library built with -DMH_DIAG, e.g. tools/ab_variants.sh build mehier.hip diag
"-DMH_DIAG"): the pictures cycle through K input sets as in bench.py (argument, default 12); tools/mehier_time.py prints the same stamps for the entry alone in a loop."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from vvcsoftware_vtm_amd.workload import Workload

rot = int(sys.argv[1]) if len(sys.argv) > 1 else 12
wl = Workload(3840, 2160, 10)
st = None
for i in range(14):
    st, out = wl.run_gpu(st, None, rotate=rot)
torch.cuda.synchronize()
os.environ["VVCGPU_MH_DIAG"] = "1"
sys.stderr.write("== stamps inside the workload, rotate %d\n" % rot)
for i in range(8):
    st, out = wl.run_gpu(st, None, rotate=rot)
torch.cuda.synchronize()
