#!/usr/bin/env python3
"""Time the precise (fp32) HaMeR route next to the default fp16 route, synthetic ViT-H weights.

Three sections, one JSON line each record:
  * "forward": device milliseconds of one HamerEngine.forward (median of --iters CUDA-event timings after --warmup) at
    B in --batches for both routes, hands/s, and the ratio of the two;
  * "family" / "gemm": one profiled precise forward at the largest B (hm_prof_*): milliseconds per kernel family (TFLOP/s
    for the GEMMs and the attention), and per GEMM shape the TFLOP/s and its fraction of the 157.3 TFLOP/s fp32 matrix peak;
  * "yardstick": hm_gemm_f32 against the fp32 tile loop it was modelled on -- hm_conv2d_nhwc with HM_DTYPE_F32, a 1x1 kernel,
    bias, no activation -- on the shapes both accept (M = 12288; (K, N) = (1024, 3840), (1024, 1280), (1024, 5120),
    (4096, 1280)), launches interleaved, median of --iters; and whether the two give the same bytes (they sum in one order).
--trace-forward B runs two precise forwards of B hands and nothing else, for a kernel trace.
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hamer_yolo_amd import lib as L  # noqa: E402
from hamer_yolo_amd import ops, synth  # noqa: E402
from hamer_yolo_amd.engine import HamerEngine  # noqa: E402

PEAK_F32 = 157.3      # TFLOP/s, fp32-input MFMA (MI355X)


def flop_per_hand(cfg) -> float:
    """GEMM and attention work of one crop through the ViT and to_kv (the decoder's one-token layers are noise next to it)."""
    v, d = cfg.vit, cfg.dec
    T, D = v.tokens, v.embed_dim
    per_block = 2 * T * D * (3 * D + D + 2 * v.mlp_ratio * D) + 4 * T * T * D
    return 2 * T * 3 * v.patch * v.patch * D + v.depth * per_block + 2 * T * D * d.depth * 2 * d.inner


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def timed(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    return float(np.median([event_ms(fn) for _ in range(iters)]))


def conv1x1_f32(x, w, bias, out):
    """hm_conv2d_nhwc, HM_DTYPE_F32, 1x1, bias, no activation, on x (M, K) seen as one 96 x (M / 96) image."""
    M, K = x.shape
    N = w.shape[0]
    a = L.ConvArgs(L.ptr(x), L.ptr(w), L.ptr(out), L.ptr(bias), None, 1, 96, M // 96, K, N, 1, 1, K, N, K, 0, 0, L.HM_DTYPE_F32)
    L.check(L.load().hm_conv2d_nhwc(C.byref(a), L.current_stream()), "hm_conv2d_nhwc")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,8,64")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--skip-forward", action="store_true")
    ap.add_argument("--trace-forward", type=int, default=0, metavar="B",
                    help="only run one warm-up and one precise forward of B hands (the program to put under rocprofv3 --kernel-trace --stats)")
    a = ap.parse_args()
    dev = "cuda:0"
    torch.cuda.set_device(0)
    if a.trace_forward:
        cfg = synth.HamerConfig()
        eng = HamerEngine(synth.hamer_state_dict(cfg, seed=0, device=dev), synth.mano_params(seed=0), cfg, device=dev, dtype=torch.float32)
        img = synth.normalize_crops(synth.crops_u8(a.trace_forward, seed0=0)).to(dev)
        for _ in range(2):
            eng.forward(img)
            torch.cuda.synchronize()
        return

    # ---- yardstick: the two fp32 tile loops on identical shapes, interleaved
    M = 12288
    for K, N in ((1024, 3840), (1024, 1280), (1024, 5120), (4096, 1280)):
        x = synth.uniform("bx", (M, K), 1.0, seed=K + N, device=dev)
        w = synth.uniform("bw", (N, K), K ** -0.5, seed=K + N + 1, device=dev)
        bias = synth.uniform("bb", (N,), 0.5, seed=3, device=dev)
        yg, yc = torch.empty(M, N, device=dev), torch.empty(M, N, device=dev)
        g = lambda: ops.gemm_f32(x, w, bias, L.HM_EPI_F32, out=yg)
        c = lambda: conv1x1_f32(x, w, bias, yc)
        for _ in range(a.warmup):
            g(); c()
        tg, tc = [], []
        for _ in range(a.iters):
            tg.append(event_ms(g)); tc.append(event_ms(c))
        torch.cuda.synchronize()
        mg, mc = float(np.median(tg)), float(np.median(tc))
        fl = 2.0 * M * N * K
        print(json.dumps({"section": "yardstick", "M": M, "K": K, "N": N, "gemm_f32_ms": round(mg, 4), "conv_f32_1x1_ms": round(mc, 4),
                          "gemm_f32_tflops": round(fl / mg / 1e9, 1), "conv_f32_tflops": round(fl / mc / 1e9, 1),
                          "gemm_over_conv_time": round(mg / mc, 3), "same_bytes": bool(torch.equal(yg, yc))}), flush=True)
        del x, w, yg, yc
    if a.skip_forward:
        return

    # ---- whole forward, both routes
    cfg = synth.HamerConfig()
    sd = synth.hamer_state_dict(cfg, seed=0, device=dev)
    mp = synth.mano_params(seed=0)
    engines = {"precise": HamerEngine(sd, mp, cfg, device=dev, dtype=torch.float32), "default": HamerEngine(sd, mp, cfg, device=dev)}
    fl = flop_per_hand(cfg)
    batches = [int(b) for b in a.batches.split(",")]
    for B in batches:
        img = synth.normalize_crops(synth.crops_u8(B, seed0=0)).to(dev)
        ms = {name: timed(lambda e=e: e.forward(img), a.warmup, a.iters) for name, e in engines.items()}
        print(json.dumps({"section": "forward", "B": B, "precise_ms": round(ms["precise"], 3), "default_ms": round(ms["default"], 3),
                          "precise_hands_per_s": round(B / ms["precise"] * 1e3, 1), "default_hands_per_s": round(B / ms["default"] * 1e3, 1),
                          "precise_over_default_time": round(ms["precise"] / ms["default"], 2),
                          "precise_tflops": round(fl * B / ms["precise"] / 1e9, 1), "gflop_per_hand": round(fl / 1e9, 1)}), flush=True)

    # ---- one profiled precise forward at the largest B: kernel families and GEMM shapes
    B = max(batches)
    img = synth.normalize_crops(synth.crops_u8(B, seed0=0)).to(dev)
    eng = engines["precise"]
    eng.forward(img)
    torch.cuda.synchronize()
    with L.profile() as prof:
        eng.forward(img)
        torch.cuda.synchronize()
    fam, gemms = {}, {}
    for kind, epi, m, n, k, ms in prof.records:
        fam[kind] = fam.get(kind, 0.0) + ms
        if kind == "gemm":
            t = gemms.setdefault((m, n, k, epi), [0.0, 0])
            t[0] += ms; t[1] += 1
    total = sum(fam.values())
    v = cfg.vit
    fam_flop = {"gemm": sum(2.0 * m * n * k * cnt for (m, n, k, _), (_, cnt) in gemms.items()),
                "attention": 4.0 * v.tokens * v.tokens * v.embed_dim * v.depth * B}
    for kind, ms in sorted(fam.items(), key=lambda kv: -kv[1]):
        rec = {"section": "family", "B": B, "kind": kind, "ms": round(ms, 3), "share": round(ms / total, 4)}
        if kind in fam_flop:
            rec["tflops"] = round(fam_flop[kind] / ms / 1e9, 1)
        print(json.dumps(rec), flush=True)
    names = {(768, 1280): "patch_embed", (1280, 3840): "qkv", (1280, 1280): "proj", (1280, 5120): "fc1", (5120, 1280): "fc2"}
    for (m, n, k, epi), (ms, cnt) in sorted(gemms.items(), key=lambda kv: -kv[1][0]):
        tf = 2.0 * m * n * k * cnt / ms / 1e9
        print(json.dumps({"section": "gemm", "B": B, "name": names.get((k, n), "to_kv"), "M": m, "N": n, "K": k, "epilogue": epi, "launches": cnt,
                          "ms_each": round(ms / cnt, 4), "tflops": round(tf, 1), "of_fp32_peak": round(tf / PEAK_F32, 3)}), flush=True)


if __name__ == "__main__":
    main()
