#!/usr/bin/env python3
"""Per-kernel register / LDS / occupancy table from hipcc's -Rpass-analysis=kernel-resource-usage remarks.

    hipcc --offload-arch=gfx950 ... -c mmidx_api.hip -o /tmp/x.o -Rpass-analysis=kernel-resource-usage 2> res.txt
    python tools/kernel_resources.py res.txt

A kernel lives in the one unit that includes its header: the search path in mmidx_api.hip, K7 / K8 (k_pca_project, k_vlad*) in
mmidx_frontend.hip, the others in mmidx_bow.hip, mmidx_learn.hip, mmidx_pca_learn.hip and mmidx_probe.hip.  The device-only
header mmidx_split16.h (the shared pieces of the bf16-split kernels) defines no kernel: its functions are inlined into K1e / K1e' /
K1e'' / K6a' (mmidx_api.hip), K8'' (mmidx_frontend.hip) and the Linear sweep (mmidx_linear.hip), so an edit there shows in all three.
"""
import re
import sys

txt = open(sys.argv[1]).read()
blocks = re.split(r"remark: [^\n]*Function Name: ", txt)[1:]
KEYS = [("vgpr", r"VGPRs"), ("agpr", r"AGPRs"), ("sgpr", r"SGPRs"), ("scratch", r"ScratchSize \[bytes/lane\]"),
        ("occ", r"Occupancy \[waves/SIMD\]"), ("lds", r"LDS Size \[bytes/block\]")]
for b in blocks:
    name = b.split("\n")[0].strip()
    vals = []
    for label, pat in KEYS:
        mm = re.search(pat + r": (\d+)", b)
        vals.append(f"{label} {mm.group(1) if mm else '?':>5}")
    print(f"{name[:70]:70s} " + " ".join(vals))
