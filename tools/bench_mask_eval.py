"""hm_mask_score against the same counts from torch ops on the same device tensors, and the render_views call it follows
(DESIGN.md section 10.2).

  python tools/bench_mask_eval.py [--frames 16 64] [--per-frame 1 4] [--rounds 10] [--warmup 3] [--log profiles/mask_eval_bench.log]

Data: N frames of 1080 x 1920 with four hand-sized meshes each (tools/bench_render.py's ellipsoids), rendered once by
``render_views``: its ``mesh_id`` is the prediction.  The mask is the same image shifted by (5, -7) pixels with label
1 + (mesh index mod 4), so every hand has a label of its own.  Radius 18 (``bound_radius(1080, 1920)``).  With one query per
frame the union of the frame's hands is scored against any label (label -1); with four, each hand against its own label.

(a) one ``mask_counts`` call (the upload of the query table, the three kernels); (b) ``torch_counts``: the rule in torch ops --
boundary maps by comparisons with replicated shifts, the disk dilation as, for every row offset dy, a horizontal run dilation
by w(dy) (a cumulative sum along x and one difference) OR-ed into the rows dy away: no convolution, no pooling; queries in
chunks of 16 to bound its memory.  (c) the ``render_views(outputs=('mesh_id',))`` call of the same frames, for scale.

A round is ``--calls`` back-to-back calls between two device events ((b): ``--torch-calls``); (a) and (b) alternate round by
round in one process after ``--warmup`` rounds of both; reported: the median round as ms per call with the fastest and slowest
round, and whether the two sides' counts are equal.  This is the time a call takes in a busy loop, host submission included.
One line per point and one JSON line go to stdout and to ``--log``."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

H, W, RADIUS, PER_FRAME = 1080, 1920, 18, 4


def torch_counts(pid, mask, queries, r, chunk=16):
    """(Q, 8) int64 on the device by torch ops alone."""
    import torch
    dev = pid.device
    hw = [max(w for w in range(r + 1) if w * w + d * d <= r * r) for d in range(r + 1)]

    def bmap(s):
        e = torch.cat([s[:, :, 1:], s[:, :, -1:]], 2)
        so = torch.cat([s[:, 1:], s[:, -1:]], 1)
        se = torch.cat([so[:, :, 1:], so[:, :, -1:]], 2)
        return (s != e) | (s != so) | (s != se)

    def dilate(b):
        Hh, Ww = b.shape[1:]
        c = torch.nn.functional.pad(torch.cumsum(b, 2, dtype=torch.int32), (r + 1, r))         # c[x + r + 1] = sum of b[..x]
        c[:, :, Ww + r + 1:] = c[:, :, Ww + r:Ww + r + 1]
        out = torch.zeros_like(b)
        for dy in range(-r, r + 1):
            w = hw[abs(dy)]
            run = (c[:, :, r + 1 + w:r + 1 + w + Ww] - c[:, :, r - w:r - w + Ww]) > 0       # some b within w along x
            if dy >= 0:
                out[:, :Hh - dy] |= run[:, dy:]
            else:
                out[:, -dy:] |= run[:, :Hh + dy]
        return out

    rows = []
    for i in range(0, len(queries), chunk):
        q = queries[i:i + chunk]
        f = torch.tensor([t[0] for t in q], device=dev)
        lo = torch.tensor([t[1] for t in q], device=dev, dtype=torch.int32)[:, None, None]
        hi = torch.tensor([t[2] for t in q], device=dev, dtype=torch.int32)[:, None, None]
        lab = torch.tensor([t[3] for t in q], device=dev, dtype=torch.int32)[:, None, None]
        p, m = pid[f], mask[f].to(torch.int32)
        pred = (p >= lo) & (p < hi)
        gt = torch.where(lab == -1, m != 0, m == lab)
        bp, bg = bmap(pred), bmap(gt)
        s = lambda t: t.sum((1, 2), dtype=torch.int64)                                       # noqa: E731
        rows.append(torch.stack([s(pred & gt), s(pred), s(gt), s(bp), s(bg), s(bp & dilate(bg)), s(bg & dilate(bp)),
                                 torch.full((len(q),), int(pid.shape[1]) * int(pid.shape[2]), dtype=torch.int64, device=dev)], 1))
    return torch.cat(rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="+", default=[16, 64])
    ap.add_argument("--per-frame", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--torch-calls", type=int, default=2)
    ap.add_argument("--render-calls", type=int, default=10)
    ap.add_argument("--log", type=str, default=os.path.join(ROOT, "profiles", "mask_eval_bench.log"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_mask_eval.py measures on the GPU; none is visible")
    from bench_render import _meshes
    from hamer_yolo_amd import render
    from hamer_yolo_amd.hamer.utils import mask_eval as ME

    def timed(fn, calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / calls

    lines, rows = [], []
    K = np.array([[1000.0, 0, W / 2], [0, 1000.0, H / 2], [0, 0, 1]])
    for N in args.frames:
        meshes = _meshes(N, PER_FRAME)
        draw = lambda: render.render_views(H, W, K, meshes, outputs=("mesh_id",), views=N)["mesh_id"]      # noqa: E731
        pid = draw()
        shifted = torch.roll(pid, (5, -7), (1, 2))
        mask = torch.where(shifted >= 0, shifted % PER_FRAME + 1, torch.zeros_like(shifted)).to(torch.uint8)
        del shifted
        torch.cuda.synchronize()
        render_ms = [timed(draw, args.render_calls) for _ in range(args.warmup + args.rounds)][args.warmup:]
        for per in args.per_frame:
            if per == 1:
                queries = [(n, n * PER_FRAME, (n + 1) * PER_FRAME, -1) for n in range(N)]
            else:
                queries = [(n, n * PER_FRAME + k, n * PER_FRAME + k + 1, k + 1) for n in range(N) for k in range(per)]
            out = torch.empty(len(queries), 8, dtype=torch.int64, device=pid.device)
            run = {"kernel": lambda: ME.mask_counts(pid, mask, queries, radius=RADIUS, counts=out),
                   "torch": lambda: torch_counts(pid, mask, queries, RADIUS)}
            calls = {"kernel": args.calls, "torch": args.torch_calls}
            k, t = run["kernel"]().clone(), run["torch"]()
            torch.cuda.synchronize()
            equal = bool(torch.equal(k, t))
            ms = {"kernel": [], "torch": []}
            for r in range(args.warmup + args.rounds):
                for name in ("kernel", "torch"):
                    v = timed(run[name], calls[name])
                    if r >= args.warmup:
                        ms[name].append(v)
            s = ME.jf_from_counts(k)
            row = {"frames": N, "queries": len(queries), "per_frame": per, "radius": RADIUS, "counts_equal_torch": equal,
                   "j_mean": float(s["J"].mean()), "f_mean": float(s["F"].mean()),
                   "boundary_pixels_per_query": float(k[:, 3:5].double().mean()),
                   "render_views_ms_per_call": round(float(np.median(render_ms)), 4),
                   "render_views_ms_min_max": [round(min(render_ms), 4), round(max(render_ms), 4)]}
            for name in ("kernel", "torch"):
                row[f"{name}_ms_per_call"] = round(float(np.median(ms[name])), 4)
                row[f"{name}_ms_min_max"] = [round(min(ms[name]), 4), round(max(ms[name]), 4)]
                row[f"{name}_calls_per_round"] = calls[name]
            row["torch_over_kernel"] = round(row["torch_ms_per_call"] / row["kernel_ms_per_call"], 2)
            rows.append(row)
            lines.append(f"{N:3d} frames x {per} queries, r = {RADIUS}: hm_mask_score {row['kernel_ms_per_call']:.4f} ms "
                         f"[{row['kernel_ms_min_max'][0]:.4f}, {row['kernel_ms_min_max'][1]:.4f}]  torch ops {row['torch_ms_per_call']:.3f} ms "
                         f"[{row['torch_ms_min_max'][0]:.3f}, {row['torch_ms_min_max'][1]:.3f}]  ({row['torch_over_kernel']}x)  "
                         f"render_views {row['render_views_ms_per_call']:.4f} ms  counts equal: {equal}")
            print(lines[-1], file=sys.stderr)
            del run, k, t
            torch.cuda.empty_cache()
        del pid, mask, meshes
        render.release_workspaces()
        ME.release_workspaces()
        torch.cuda.empty_cache()
    lines.append(json.dumps({"bench": "mask_eval", "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "warmup": args.warmup,
                             "size": [H, W], "rows": rows}))
    print("\n".join(lines))
    if args.log:
        with open(args.log, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
