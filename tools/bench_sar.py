#!/usr/bin/env python3
"""Time the SAR hand-mesh head (SarHeadEngine.forward: SAIGB, both GBBMR branches, mesh2pose + soft-argmax) and the
end-to-end estimator on prepared patches (ResNet-34 features + head + ResRootNet + post-process, what run_frames does after
the crops) at B = 1 / 64 / 256 hands, synthetic weights.  Prints one JSON line per batch size with device milliseconds
(median of --iters CUDA-event timings after --warmup) and the head's TFLOP/s.  --precise times the fp32 route
(EstimateRGB(cfg, precise=True)) instead and adds "route" and the backbone's TFLOP/s to each line.  --backbone convnext times
the ConvNeXt-base SAR (ConvNextEngine + the 1024-channel head) the same way, with the backbone's TFLOP/s on 40.1 GFLOP per
hand."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hamer_yolo_amd import synth  # noqa: E402
from hamer_yolo_amd.rootnet.engine import RootNetEngine  # noqa: E402
from hamer_yolo_amd.rootnet.sar import SarHeadEngine, sar_hand  # noqa: E402

NV = 778


def head_flop_per_hand():
    saigb = 2 * 8 * NV * 512 * 64
    branch = 2 * NV * NV * (515 + 1024) + 2 * NV * 1024 * (515 + 1024)
    return saigb + 2 * branch + 2 * 2 * 21 * NV * 1024


def backbone_flop_per_hand():
    """The ResNet-34 convolutions on a 256 x 256 patch (the 7x7 stem on the 8-channel image as the kernel runs it)."""
    from hamer_yolo_amd.rootnet import arch
    fl = 2 * 128 * 128 * 64 * 7 * 7 * 8
    hw = 64
    for _, cin, cout, s, ds in arch.blocks():
        ho = hw // s
        fl += 2 * ho * ho * cout * 9 * cin + 2 * ho * ho * cout * 9 * cout + (2 * ho * ho * cout * cin if ds else 0)
        hw = ho
    return fl


def timed(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,64,256")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--precise", action="store_true", help="time the fp32 route (backbone, RootNet and head in fp32)")
    ap.add_argument("--backbone", choices=("resnet34", "convnext", "both"), default="resnet34",
                    help="both: the ResNet-34 lines, then the ConvNeXt lines, from one process")
    a = ap.parse_args()
    if a.precise and a.backbone != "resnet34":
        ap.error("the fp32 route of the convnext backbone does not exist yet")
    for backbone in (("resnet34", "convnext") if a.backbone == "both" else (a.backbone,)):
        run(a, backbone)


def run(a, backbone):
    dev = "cuda:0"
    convnext = backbone == "convnext"
    if convnext:
        from hamer_yolo_amd.rootnet import convnext_arch
        from hamer_yolo_amd.rootnet.convnext_engine import ConvNextEngine
        bb = ConvNextEngine(synth.convnext_state_dict(0), synth.convnext_rootnet_state_dict(0), device=dev)
        head = SarHeadEngine(synth.sar_head_state_dict(0, in_channels=1024), device=dev, in_channels=1024)
    else:
        net, root = synth.rootnet_state_dict(0)
        bb = RootNetEngine(net, root, device=dev, dtype=torch.float32 if a.precise else torch.float16)
        head = SarHeadEngine(synth.sar_head_state_dict(0), device=dev, precise=a.precise)
    K = np.array([[906.96, 0, 960], [0, 906.79, 540], [0, 0, 1]])
    for B in [int(x) for x in a.batches.split(",")]:
        img = torch.randn(B, 3, 256, 256, device=dev)
        feat = bb.features(img)
        kv = torch.full((B,), 1.5, device=dev)
        hands = [sar_hand(np.array([[0.7, 0, 500.0], [0, 0.7, 300.0]], np.float32), K, 1920, 1080, False)] * B

        def e2e():
            f = bb.features(img)
            c = head.forward(f)
            head.postprocess(c, hands, bb.depth_of(f, kv))
        t_head = timed(lambda: head.forward(feat), a.warmup, a.iters)
        t_bb = timed(lambda: bb.features(img), a.warmup, a.iters)
        t_e2e = timed(e2e, a.warmup, a.iters)
        rec = {"B": B, "head_ms": round(t_head, 4), "head_tflops": round(head_flop_per_hand() * B / t_head / 1e9, 1),
               "backbone_ms": round(t_bb, 4), "end_to_end_ms": round(t_e2e, 4),
               "head_gflop_per_hand": round(head_flop_per_hand() / 1e9, 2)}
        if a.precise:
            rec = {"route": "precise", **rec, "backbone_tflops": round(backbone_flop_per_hand() * B / t_bb / 1e9, 1),
                   "backbone_gflop_per_hand": round(backbone_flop_per_hand() / 1e9, 2)}
        if convnext:
            # (SAIGB's K is 1024 here: twice its flops in the head's count)
            rec = {"backbone": "convnext", **rec, "backbone_tflops": round(convnext_arch.GFLOP_PER_HAND * B / t_bb, 1),
                   "backbone_gflop_per_hand": convnext_arch.GFLOP_PER_HAND,
                   "head_tflops": round((head_flop_per_hand() + 2 * 8 * NV * 512 * 64) * B / t_head / 1e9, 1)}
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
