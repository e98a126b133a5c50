#!/usr/bin/env python3
"""Per-kernel register / spill / LDS report of one HIP source (hipcc -Rpass-analysis=kernel-resource-usage, gfx950).
Usage: python tools/kernel_resources.py hamer_yolo_amd/csrc/gemm.hip [name-filter]"""
import re
import subprocess
import sys

src = sys.argv[1]
flt = sys.argv[2] if len(sys.argv) > 2 else ""
out = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-c", src, "-o", "/dev/null",
                      "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True).stderr
cur = None
rows = {}
for line in out.splitlines():
    m = re.search(r"remark:\s+(Function Name|VGPRs|AGPRs|VGPRs Spill|TotalSGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]):\s+(\S+)", line)
    if not m:
        continue
    k, v = m.groups()
    if k == "Function Name":
        cur = subprocess.run(["c++filt", v], capture_output=True, text=True).stdout.strip()
        rows[cur] = {}
    elif cur:
        rows[cur][k.split(" [")[0]] = v
for name, r in rows.items():
    if flt in name:
        short = name.replace("(anonymous namespace)::", "")
        print(f"{short[:110]:110s} vgpr {r.get('VGPRs','?'):>4} agpr {r.get('AGPRs','?'):>3} sgpr {r.get('TotalSGPRs','?'):>3} spill {r.get('VGPRs Spill','?'):>3} "
              f"scratch {r.get('ScratchSize','?'):>4} lds {r.get('LDS Size','?'):>6} occ {r.get('Occupancy','?')}")
