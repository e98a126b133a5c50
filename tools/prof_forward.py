#!/usr/bin/env python3
"""Serial HaMeR forwards at B = 64 (one batch in flight) under one value of HM_OPT_GEMM_STAGGER, for a profiler run:
`rocprofv3 --kernel-trace --stats -- python3 tools/prof_forward.py`.  Env: STAGGER=0|1|2 (default 0), STEPS=10, WARMUP=3."""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from hamer_yolo_amd import lib as L
from hamer_yolo_amd import synth
from hamer_yolo_amd.engine import HamerEngine
from runlog import banner

banner()
steps, warmup, B = int(os.environ.get("STEPS", 10)), int(os.environ.get("WARMUP", 3)), int(os.environ.get("BATCH", 64))
cfg = synth.HamerConfig()
eng = HamerEngine(synth.hamer_state_dict(cfg, seed=0, device="cuda"), synth.mano_params(seed=0), cfg)
img = synth.normalize_crops(synth.crops_u8(B, seed0=0)).cuda()
L.check(L.load().hm_set_option(L.HM_OPT_GEMM_STAGGER, int(os.environ.get("STAGGER", 0))))
for _ in range(warmup):
    eng.forward(img)
torch.cuda.synchronize()
t0 = time.perf_counter()
for _ in range(steps):
    eng.forward(img)
torch.cuda.synchronize()
print(f"stagger={os.environ.get('STAGGER', 0)} {(time.perf_counter() - t0) / steps * 1e3:.3f} ms/step")
