"""The HaMeR crop launches side by side: hm_crop_batch (the default, no prefilter) and hm_crop_batch_aa
(--antialias-crop) on one seeded 1080p noise frame, 64 hands per launch, every hand a square crop of side S with a seeded
centre inside the frame and alternating labels.

  python tools/bench_crop.py [--hands 64] [--sizes 400 700 1000 2000 5000] [--rounds 20] [--launches 10]

Per S: device-event time of ``--launches`` back-to-back launches, the two entry points alternating round by round in one
process after a warm-up of both; the median over the rounds is reported as ms per launch, with the fastest and slowest round.
``footprint_mb`` is what the algorithm has to read: per hand the frame bytes under the crop square grown by the blur radius + 1,
clipped to the frame; ``aa_gbs`` is that over the launch time (a rate of needed bytes, not of issued loads -- the kernel reads
every needed byte once per output row that uses it).  S = 400 takes the 8-bit rule inside hm_crop_batch_aa.  One JSON line."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hamer_yolo_amd import ops  # noqa: E402

H, W, P = 1080, 1920, 256
MEAN = 255.0 * np.array([0.485, 0.456, 0.406])
STD = 255.0 * np.array([0.229, 0.224, 0.225])


def blur_radius(S):
    df = (S / P) / 2.0
    return int(4.0 * ((df - 1) / 2) + 0.5) if df > 1.1 else 0


def footprint_bytes(boxes):
    total = 0
    for cx, cy, S, _ in boxes:
        g = blur_radius(S) + 1
        w = max(0.0, min(W, cx + S / 2 + g) - max(0.0, cx - S / 2 - g))
        h = max(0.0, min(H, cy + S / 2 + g) - max(0.0, cy - S / 2 - g))
        total += w * h * 3
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hands", type=int, default=64)
    ap.add_argument("--sizes", type=float, nargs="+", default=[400, 700, 1000, 2000, 5000])
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--launches", type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_crop.py measures on the GPU; none is visible")
    rng = np.random.default_rng(0)
    frame = torch.from_numpy(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).cuda()
    out = torch.empty(args.hands, 3, P, P, device="cuda")
    rows = []
    for S in args.sizes:
        boxes = [(float(rng.uniform(0.2, 0.8) * W), float(rng.uniform(0.2, 0.8) * H), float(S), i % 2 == 1) for i in range(args.hands)]
        rec, rec_aa = ops.crop_boxes(boxes, P).cuda(), ops.crop_boxes_aa(boxes, P).cuda()
        run = {"plain": lambda: ops.crop_batch(frame, rec, MEAN, STD, P, out=out),
               "aa": lambda: ops.crop_batch_aa(frame, rec_aa, MEAN, STD, P, out=out)}
        for f in run.values():
            for _ in range(3):
                f()
        torch.cuda.synchronize()
        ms = {"plain": [], "aa": []}
        for _ in range(args.rounds):
            for name, f in run.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(args.launches):
                    f()
                b.record()
                b.synchronize()
                ms[name].append(a.elapsed_time(b) / args.launches)
        fb = footprint_bytes(boxes)
        row = {"S": S, "radius": blur_radius(S), "footprint_mb": round(fb / 1e6, 2)}
        for name in ("plain", "aa"):
            v = sorted(ms[name])
            row[name + "_ms"] = round(v[len(v) // 2], 4)
            row[name + "_ms_range"] = [round(v[0], 4), round(v[-1], 4)]
        row["aa_gbs"] = round(fb / (row["aa_ms"] * 1e-3) / 1e9, 1)
        rows.append(row)
        print(f"S {S:6.0f} r {row['radius']:2d}: hm_crop_batch {row['plain_ms']:.4f} ms  hm_crop_batch_aa {row['aa_ms']:.4f} ms "
              f"{row['aa_ms_range']}  footprint {row['footprint_mb']} MB -> {row['aa_gbs']} GB/s", file=sys.stderr)
    print(json.dumps({"bench": "crop", "frame": [H, W], "hands": args.hands, "launches": args.launches, "rounds": args.rounds, "rows": rows}))


if __name__ == "__main__":
    main()
