"""hm_mesh_penetration on hand-sized meshes, overlapping and disjoint, next to hm_mesh_score on the same point counts
(DESIGN.md section 10.7).

  python tools/bench_penetration.py [--queries 16 64 256] [--rounds 6] [--warmup 2] [--calls 20] [--log profiles/penetration_bench.log]

Data: Q / 2 pairs of closed lat-lon ellipsoids of 778 vertices and 1552 faces (the MANO mesh closed at the wrist has 778 and
1554), both directions of every pair: Q queries.  OVERLAPPING: the second mesh 3 cm beside the first, so the boxes overlap, b's
faces are staged and every vertex inside b's inflated box meets every face.  DISJOINT: the second mesh 30 cm away, the early
out: the workgroups write FAR and leave.  As a scale, ``mesh_score`` (hm_mesh_score: all pairwise point distances of two sets of
778 points, Q pairs) in the same run.

Each is timed through its Python wrapper: a round is ``--calls`` back-to-back calls between two device events; the three
alternate round by round in one process after ``--warmup`` rounds of each; reported: the median round as ms per call with the
fastest and slowest round.  This is the time a call takes in a busy loop, host submission (packing the mesh table, the
concatenation of the vertex arrays) included.  Next to it the DEVICE time of the call alone (its memset and launches between
two events of the library's profiler, ``lib.profile``): the median of ``--calls`` calls.  There is no pass mark: the parent
commit has no such call.  One line per point and one JSON line go to stdout and to ``--log``.

Measured on an MI355X (profiles/penetration_bench.log, one run): overlapping 16 queries 0.318 ms per call (0.309 ms of it on the device), 64 queries 0.548 ms (0.525 ms), 256 queries 1.610 ms (1.311 ms);
disjoint queries, the early out, 0.143 / 0.428 / 1.545 ms per call of which 0.025 / 0.027 / 0.049 ms on the device;
hm_mesh_score 0.163 / 0.167 / 0.182 ms.  DESIGN.md section 10.7."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, nargs="+", default=[16, 64, 256])
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--log", type=str, default=os.path.join(ROOT, "profiles", "penetration_bench.log"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_penetration.py measures on the GPU; none is visible")
    from depth_eval_rule import ellipsoid
    from hamer_yolo_amd import lib as L
    from hamer_yolo_amd.hamer.utils import penetration as PN
    from hamer_yolo_amd.hamer.utils.mesh_eval import mesh_score
    dev = torch.device("cuda", 0)

    def timed(fn, calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / calls

    def device_ms(fn, calls):
        with L.profile(capacity=4 * calls) as prof:
            for _ in range(calls):
                fn()
            torch.cuda.synchronize()
        ms = sorted(r[-1] for r in prof.records)
        return ms[len(ms) // 2]

    v, f = ellipsoid((0.04, 0.09, 0.015), n_lat=9, n_lon=97)
    assert v.shape == (778, 3) and f.shape == (1552, 3)
    faces = torch.from_numpy(f).to(dev)
    rng = np.random.default_rng(0)
    lines, rows = [], []
    for Q in args.queries:
        def scene(gap):
            out = []
            for p in range(Q // 2):
                c = rng.uniform(-0.2, 0.2, 3) + (0.0, 0.0, 0.6)
                for k in (0, 1):
                    out.append({"frame": p, "vertices": torch.from_numpy(v + c + (gap * k, 0.004 * k, 0.003 * k)).to(dev), "faces": faces})
            return out
        over, apart = scene(0.03), scene(0.30)
        pred = torch.stack([m["vertices"] for m in over]).to(torch.float32).contiguous()
        gt = torch.stack([over[i ^ 1]["vertices"] for i in range(Q)]).to(torch.float32).contiguous()
        run = {"overlapping": lambda: PN.hand_penetration(over), "disjoint": lambda: PN.hand_penetration(apart),
               "mesh_score": lambda: mesh_score(pred, gt)}
        first = {k: fn() for k, fn in run.items()}
        torch.cuda.synchronize()
        so, sa = PN.summary(first["overlapping"]["sums"]), PN.summary(first["disjoint"]["sums"])
        ok = bool((so["status"] == 0).all() and (so["inside"] > 0).all() and (sa["status"] == 1).all() and (sa["tested"] == 0).all())
        ms = {k: [] for k in run}
        for rd in range(args.warmup + args.rounds):
            for name in run:
                t = timed(run[name], args.calls)
                if rd >= args.warmup:
                    ms[name].append(t)
        row = {"queries": Q, "vertices_per_query": 778, "faces_per_query": 1552, "tested_vertices": int(so["tested"].sum()),
               "inside_vertices": int(so["inside"].sum()), "max_depth_m": float(so["max_depth_m"].max()), "as_expected": ok}
        for name in run:
            row[f"{name}_ms_per_call"] = round(float(np.median(ms[name])), 4)
            row[f"{name}_ms_min_max"] = [round(min(ms[name]), 4), round(max(ms[name]), 4)]
        for name in ("overlapping", "disjoint"):
            row[f"{name}_device_ms"] = round(float(device_ms(run[name], args.calls)), 4)
        rows.append(row)
        lines.append(f"{Q:3d} queries of 778 vertices x 1552 faces: overlapping {row['overlapping_ms_per_call']:.4f} ms "
                     f"[{row['overlapping_ms_min_max'][0]:.4f}, {row['overlapping_ms_min_max'][1]:.4f}], on the device {row['overlapping_device_ms']:.4f} ms "
                     f"({row['tested_vertices']} vertices tested, "
                     f"{row['inside_vertices']} inside)  disjoint {row['disjoint_ms_per_call']:.4f} ms [{row['disjoint_ms_min_max'][0]:.4f}, "
                     f"{row['disjoint_ms_min_max'][1]:.4f}], on the device {row['disjoint_device_ms']:.4f} ms  hm_mesh_score of {Q} x 778 x 778 points {row['mesh_score_ms_per_call']:.4f} ms  "
                     f"as expected: {ok}")
        print(lines[-1], file=sys.stderr)
        del run, first, over, apart, pred, gt
        PN.release_workspaces()
    lines.append(json.dumps({"bench": "penetration", "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "warmup": args.warmup,
                             "calls": args.calls, "rows": rows}))
    print("\n".join(lines))
    if args.log:
        os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
        with open(args.log, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
