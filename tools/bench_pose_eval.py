"""hm_pose_eval against the same computation in torch ops on the same device tensors.

  python tools/bench_pose_eval.py [--batches 64 1024] [--points 21 778] [--rounds 10] [--warmup 3] [--calls 2000] [--torch-calls 100]
  rocprofv3 --kernel-trace -d DIR -o pe --output-format csv -- python tools/bench_pose_eval.py --trace-calls 20
  python tools/bench_pose_eval.py --parse-trace DIR/.../pe_kernel_trace.csv --trace-calls 20

Per (B, N): MPJPE and PA-MPJPE of B seeded hand-sized point sets, by (a) one hm_pose_eval launch and (b) the torch-ops chain of
tests/pose_eval_rule.torch_chain (the reference's pose_utils.py with torch.linalg.svd for the deprecated torch.svd), neither
copying anything to the host.

Timed mode.  A round is ``--calls`` (kernel) or ``--torch-calls`` (torch ops) back-to-back calls between two device events -- tens
of milliseconds per window; the two sides alternate round by round in one process after ``--warmup`` rounds of both; reported:
the median round over ``--rounds`` as ms per call, with the fastest and slowest round, and the largest difference between the
two sides' results.  This is the time a CALL takes in a busy loop, host submission included (for the kernel side: the Python
wrapper, a ctypes struct and one launch); it is not the kernel's own time.

Trace mode (``--trace-calls K``; under rocprofv3 --kernel-trace).  Per (B, N): one warm call of each side, then K kernel calls,
then K torch calls, nothing timed.  ``--parse-trace`` reads the kernel trace back: per point the median duration of the K
pose_eval_kernel dispatches (the kernel's own time), and for the torch side the number of kernels per call and their summed
duration per call (device-busy time, gaps between launches excluded).  One JSON line either way."""
import argparse
import csv
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def points_of(args):
    return [(B, N) for B in args.batches for N in args.points]


def parse_trace(path, pts, K):
    with open(path) as f:
        rows = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(f))
    ours = [i for i, r in enumerate(rows) if "pose_eval_kernel" in r[2]]
    if len(ours) != len(pts) * (K + 1):
        raise SystemExit(f"{path}: {len(ours)} pose_eval_kernel dispatches, expected {len(pts) * (K + 1)}")
    out = []
    for p, (B, N) in enumerate(pts):
        mine = ours[p * (K + 1):(p + 1) * (K + 1)]
        kernel_us = [(rows[i][1] - rows[i][0]) / 1e3 for i in mine[1:]]              # the first one is the warm call
        end = ours[(p + 1) * (K + 1)] if p + 1 < len(pts) else len(rows)
        torch_rows = rows[mine[-1] + 1:end]                                         # the K torch calls that follow
        out.append({"B": B, "N": N, "kernel_us": round(float(np.median(kernel_us)), 2),
                    "kernel_us_min_max": [round(min(kernel_us), 2), round(max(kernel_us), 2)],
                    "torch_kernels_per_call": round(len(torch_rows) / K, 1),
                    "torch_device_busy_us_per_call": round(sum(e - s for s, e, _ in torch_rows) / 1e3 / K, 1)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[64, 1024])
    ap.add_argument("--points", type=int, nargs="+", default=[21, 778])
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=2000)
    ap.add_argument("--torch-calls", type=int, default=100)
    ap.add_argument("--trace-calls", type=int, default=0)
    ap.add_argument("--parse-trace", type=str, default=None)
    args = ap.parse_args()
    if args.parse_trace:
        print(json.dumps({"bench": "pose_eval_trace", "calls": args.trace_calls, "rows": parse_trace(args.parse_trace, points_of(args), args.trace_calls)}))
        return
    import torch
    import pose_eval_rule as PR
    from hamer_yolo_amd.hamer.utils import pose_utils as PU
    if not torch.cuda.is_available():
        raise SystemExit("bench_pose_eval.py measures on the GPU; none is visible")

    def timed(fn, calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / calls

    rows = []
    for B, N in points_of(args):
        rng = np.random.default_rng(B * 10000 + N)
        gt = rng.normal(size=(B, N, 3)) * 0.04 + rng.normal(size=(B, 1, 3)) * 0.1 + np.array([0.0, 0.0, 0.5])
        pred = gt + rng.normal(size=(B, N, 3)) * 0.008 + rng.normal(size=(B, 1, 3)) * 0.02
        pred, gt = torch.tensor(pred, dtype=torch.float32).cuda(), torch.tensor(gt, dtype=torch.float32).cuda()
        err, pa = torch.empty(B, device="cuda"), torch.empty(B, device="cuda")
        run = {"kernel": lambda: PU.pose_eval(pred, gt, err=err, pa_err=pa), "torch": lambda: PR.torch_chain(pred, gt)}
        calls = {"kernel": args.calls, "torch": args.torch_calls}
        k, t = run["kernel"](), run["torch"]()
        torch.cuda.synchronize()
        if args.trace_calls:
            for name in ("kernel", "torch"):
                for _ in range(args.trace_calls):
                    run[name]()
                torch.cuda.synchronize()
            continue
        diff = max(float((k["err"] - t[0]).abs().max()), float((k["pa_err"] - t[1]).abs().max()))
        ms = {"kernel": [], "torch": []}
        for r in range(args.warmup + args.rounds):
            for name in ("kernel", "torch"):
                v = timed(run[name], calls[name])
                if r >= args.warmup:
                    ms[name].append(v)
        row = {"B": B, "N": N, "max_abs_diff_m": diff}
        for name in ("kernel", "torch"):
            row[f"{name}_ms_per_call"] = round(float(np.median(ms[name])), 5)
            row[f"{name}_ms_min_max"] = [round(min(ms[name]), 5), round(max(ms[name]), 5)]
            row[f"{name}_window_ms"] = round(float(np.median(ms[name])) * calls[name], 1)
        row["torch_over_kernel"] = round(row["torch_ms_per_call"] / row["kernel_ms_per_call"], 2)
        rows.append(row)
        print(f"B {B:5d} N {N:4d}: kernel call {row['kernel_ms_per_call']:.4f} ms  torch ops {row['torch_ms_per_call']:.4f} ms  "
              f"({row['torch_over_kernel']}x)  max |diff| {diff:.3g} m", file=sys.stderr)
    if args.trace_calls:
        print(json.dumps({"bench": "pose_eval", "mode": "trace", "calls": args.trace_calls}))
        return
    print(json.dumps({"bench": "pose_eval", "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "warmup": args.warmup,
                      "calls_per_round": {"kernel": args.calls, "torch": args.torch_calls}, "rows": rows}))


if __name__ == "__main__":
    main()
