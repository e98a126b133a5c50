"""hm_mesh_score and hm_pck_auc against the same computations in torch ops on the same device tensors.

  python tools/bench_mesh_eval.py [--batches 64 1024] [--samples 64 10000] [--keypoints 21 799] [--rounds 10] [--warmup 3]
  rocprofv3 --kernel-trace -d DIR -o me --output-format csv -- python tools/bench_mesh_eval.py --trace-calls 20
  python tools/bench_mesh_eval.py --parse-trace DIR/.../me_kernel_trace.csv --trace-calls 20

F-score points: B hands of 778 x 778 seeded hand-sized clouds, F@5 mm and F@15 mm, by (a) one hm_mesh_score launch and (b) the
torch-ops chain of tests/mesh_eval_rule.torch_f_score -- an fp64 broadcast distance matrix, two minima, the comparisons.  AUC
points: N x K seeded joint errors, 100 thresholds over 0-50 mm, by (a) one hm_pck_auc call (the zeroing of its workspace, the
histogram kernel, the finishing workgroup) and (b) tests/mesh_eval_rule.torch_auc -- (err[..., None] <= thr).double().mean(0)
plus trapezoids.  Neither side copies anything to the host.

Timed mode.  A round is a number of back-to-back calls between two device events (``--calls`` / ``--torch-calls``; the torch
F-score chain at B = 1024 allocates tens of GB per call and gets ``--big-torch-calls``); the two sides alternate round by round
in one process after ``--warmup`` rounds of both; reported: the median round over ``--rounds`` as ms per call, with the fastest
and slowest round, and the largest difference between the two sides' results.  This is the time a CALL takes in a busy loop,
host submission included (for the kernel side: the Python wrapper, output allocation, a ctypes struct and the launches); it is
not the kernel's own time.

Trace mode (``--trace-calls K``; under rocprofv3 --kernel-trace).  Per point: one warm call of each side, then K kernel-side
calls, then K torch calls, nothing timed.  ``--parse-trace`` reads the kernel trace back: per point the median device time of a
kernel-side call over the last K - 1 of them (every dispatch between two calls' last kernels, so the workspace fill counts), and
for the torch side the number of kernels per call and their summed duration per call.  One JSON line either way."""
import argparse
import csv
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

N_VERTS, STEPS, THR = 778, 100, (0.005, 0.015)
OURS = ("mesh_score_kernel", "pck_hist_kernel", "pck_finish_kernel")
LAST = ("mesh_score_kernel", "pck_finish_kernel")                        # the last kernel of a kernel-side call


def points_of(args):
    return [("fscore", B, N_VERTS) for B in args.batches] + [("auc", N, K) for N in args.samples for K in args.keypoints]


def parse_trace(path, pts, K):
    with open(path) as f:
        rows = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(f))
    marks = [i for i, r in enumerate(rows) if any(n in r[2] for n in LAST)]
    if len(marks) != len(pts) * (K + 1):
        raise SystemExit(f"{path}: {len(marks)} kernel-side calls, expected {len(pts) * (K + 1)}")
    out = []
    for p, (kind, a, b) in enumerate(pts):
        mine = marks[p * (K + 1):(p + 1) * (K + 1)]                         # the warm call, then the K traced ones
        call_us = [sum(e - s for s, e, _ in rows[mine[i - 1] + 1:mine[i] + 1]) / 1e3 for i in range(2, K + 1)]
        end = marks[(p + 1) * (K + 1)] if p + 1 < len(pts) else len(rows)
        torch_rows = [r for r in rows[mine[-1] + 1:end] if not any(n in r[2] for n in OURS) and "fillBuffer" not in r[2]]
        out.append({"kind": kind, "B_or_N": a, "points_or_K": b, "kernel_side_us": round(float(np.median(call_us)), 2),
                    "kernel_side_us_min_max": [round(min(call_us), 2), round(max(call_us), 2)],
                    "dispatches_per_kernel_side_call": round((mine[-1] - mine[1]) / (K - 1), 1),
                    "torch_kernels_per_call": round(len(torch_rows) / K, 1),
                    "torch_device_busy_us_per_call": round(sum(e - s for s, e, _ in torch_rows) / 1e3 / K, 1)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[64, 1024])
    ap.add_argument("--samples", type=int, nargs="+", default=[64, 10000])
    ap.add_argument("--keypoints", type=int, nargs="+", default=[21, 799])
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--torch-calls", type=int, default=20)
    ap.add_argument("--big-torch-calls", type=int, default=2)
    ap.add_argument("--trace-calls", type=int, default=0)
    ap.add_argument("--parse-trace", type=str, default=None)
    args = ap.parse_args()
    if args.parse_trace:
        print(json.dumps({"bench": "mesh_eval_trace", "calls": args.trace_calls, "rows": parse_trace(args.parse_trace, points_of(args), args.trace_calls)}))
        return
    import torch
    import mesh_eval_rule as MR
    from hamer_yolo_amd.hamer.utils import mesh_eval as ME
    if not torch.cuda.is_available():
        raise SystemExit("bench_mesh_eval.py measures on the GPU; none is visible")

    def timed(fn, calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / calls

    rows = []
    for kind, a, b in points_of(args):
        rng = np.random.default_rng(a * 10000 + b)
        if kind == "fscore":
            gt = rng.normal(size=(a, b, 3)) * 0.04 + rng.normal(size=(a, 1, 3)) * 0.1 + np.array([0.0, 0.0, 0.5])
            pred = gt + rng.normal(size=(a, b, 3)) * 0.008 + rng.normal(size=(a, 1, 3)) * 0.004
            pred, gt = torch.tensor(pred, dtype=torch.float32).cuda(), torch.tensor(gt, dtype=torch.float32).cuda()
            out = {"fscore": torch.empty(a, len(THR), device="cuda")}
            run = {"kernel": lambda: ME.mesh_score(pred, gt, thresholds=THR, want=(), out=out)["fscore"],
                   "torch": lambda: MR.torch_f_score(pred, gt, THR)}
            calls = {"kernel": args.calls, "torch": args.big_torch_calls if a > 256 else args.torch_calls}
        else:
            err = torch.tensor(rng.gamma(2.0, 0.008, size=(a, b)), dtype=torch.float32).cuda()
            run = {"kernel": lambda: ME.pck_auc(err, 0.0, 0.05, STEPS)["mean_auc"][0], "torch": lambda: MR.torch_auc(err, 0.0, 0.05, STEPS)[0]}
            calls = {"kernel": args.calls, "torch": args.torch_calls}
        k, t = run["kernel"](), run["torch"]()
        torch.cuda.synchronize()
        if args.trace_calls:
            for name in ("kernel", "torch"):
                for _ in range(args.trace_calls):
                    run[name]()
                torch.cuda.synchronize()
            continue
        diff = float((k.double() - t).abs().max())
        ms = {"kernel": [], "torch": []}
        for r in range(args.warmup + args.rounds):
            for name in ("kernel", "torch"):
                v = timed(run[name], calls[name])
                if r >= args.warmup:
                    ms[name].append(v)
        row = {"kind": kind, "B_or_N": a, "points_or_K": b, "max_abs_diff": diff}
        for name in ("kernel", "torch"):
            row[f"{name}_ms_per_call"] = round(float(np.median(ms[name])), 5)
            row[f"{name}_ms_min_max"] = [round(min(ms[name]), 5), round(max(ms[name]), 5)]
            row[f"{name}_calls_per_round"] = calls[name]
        row["torch_over_kernel"] = round(row["torch_ms_per_call"] / row["kernel_ms_per_call"], 2)
        rows.append(row)
        print(f"{kind:6s} {a:5d} x {b:4d}: kernel side {row['kernel_ms_per_call']:.4f} ms  torch ops {row['torch_ms_per_call']:.4f} ms  "
              f"({row['torch_over_kernel']}x)  max |diff| {diff:.3g}", file=sys.stderr)
        del run, k, t
        torch.cuda.empty_cache()
    if args.trace_calls:
        print(json.dumps({"bench": "mesh_eval", "mode": "trace", "calls": args.trace_calls}))
        return
    print(json.dumps({"bench": "mesh_eval", "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "warmup": args.warmup,
                      "steps": STEPS, "thresholds_m": list(THR), "rows": rows}))


if __name__ == "__main__":
    main()
