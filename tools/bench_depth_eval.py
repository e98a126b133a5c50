"""hm_depth_residuals against the same histograms from torch ops on the same device tensors, its rate over the pred_id bytes it
reads, and two iterations of refine_cam_t.

  python tools/bench_depth_eval.py [--frames 16 64] [--per-frame 1 4] [--rounds 10] [--warmup 3] [--log profiles/depth_eval_bench.log]

Data: N frames of 1080 x 1920 with four hand-sized meshes each (tools/bench_render.py's ellipsoids), rendered once by
``render_views``: its ``depth`` and ``mesh_id`` are the prediction.  The sensor image is that depth plus 10 mm in millimetres,
a wall at 1.5 m where nothing is covered, shifted by (5, -7) pixels so that the footprints do not agree.  With one query per
frame the frame's four meshes share it; with four, each mesh has its own.

(a) one ``depth_residuals`` call (the upload of the mesh table, the three kernels); (b) ``torch_hist``: the rule in torch ops --
per query a boolean mask of its frame, the residual in fp64, the floor of its quotient by the bin width and ``bincount``.
(c) ``refine_cam_t`` with two iterations over the N frames' 4 N hands: two ``render_views`` calls, two ``depth_residuals`` calls
and the update.

A round is ``--calls`` back-to-back calls between two device events ((b): ``--torch-calls``, (c): ``--refine-calls``); (a) and
(b) alternate round by round in one process after ``--warmup`` rounds of both; reported: the median round as ms per call with
the fastest and slowest round, whether the two sides' histograms are equal, and the N H W 4 bytes of pred_id over (a)'s time
next to hm_mask_boxes' rate over its N H W bytes (profiles/mask_boxes_bench.log).  This is the time a call takes in a busy
loop, host submission included.  One line per point and one JSON line go to stdout and to ``--log``."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

H, W, PER_FRAME, UNIT, BIN_M, BINS = 1080, 1920, 4, 0.001, 0.0005, 4096
MASK_BOXES_TB_S = {16: 2.140, 64: 4.483}          # profiles/mask_boxes_bench.log, one query per frame


def torch_hist(depth, pid, sensor, groups):
    """(Q, BINS) int64 on the device by torch ops alone; ``groups``: per query (frame, id_lo, id_hi)."""
    import torch
    rows = []
    for n, lo, hi in groups:
        p, raw = pid[n], sensor[n].to(torch.int32)
        sel = (p >= lo) & (p < hi) & (raw != 0)
        r = raw.to(torch.float64) * UNIT - depth[n].to(torch.float64)
        k = torch.floor(r / BIN_M).to(torch.int64) + BINS // 2      # (floor_divide corrects by the remainder: not the rule on an edge)
        k = k[sel & (k >= 0) & (k < BINS)]
        rows.append(torch.bincount(k, minlength=BINS))
    return torch.stack(rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="+", default=[16, 64])
    ap.add_argument("--per-frame", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--torch-calls", type=int, default=2)
    ap.add_argument("--refine-calls", type=int, default=3)
    ap.add_argument("--refine-frames", type=int, default=64)
    ap.add_argument("--log", type=str, default=os.path.join(ROOT, "profiles", "depth_eval_bench.log"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_depth_eval.py measures on the GPU; none is visible")
    from bench_render import _meshes, surface_mesh
    from hamer_yolo_amd import render
    from hamer_yolo_amd.hamer.utils import depth_eval as DE

    def timed(fn, calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / calls

    def sensor_of(depth):
        mm = torch.round(torch.where(depth > 0, depth + 0.010, torch.full_like(depth, 1.5)) / UNIT).to(torch.int32).to(torch.int16)
        return torch.roll(mm, (5, -7), (1, 2)).contiguous()

    lines, rows = [], []
    K = np.array([[1000.0, 0, W / 2], [0, 1000.0, H / 2], [0, 0, 1]])
    for N in args.frames:
        r = render.render_views(H, W, K, _meshes(N, PER_FRAME), outputs=("depth", "mesh_id"), views=N)
        depth, pid = r["depth"], r["mesh_id"]
        sensor = sensor_of(depth)
        torch.cuda.synchronize()
        for per in args.per_frame:
            if per == 1:
                mq = [n for n in range(N) for _ in range(PER_FRAME)]
                groups = [(n, n * PER_FRAME, (n + 1) * PER_FRAME) for n in range(N)]
            else:
                mq = list(range(N * PER_FRAME))
                groups = [(n, n * PER_FRAME + k, n * PER_FRAME + k + 1) for n in range(N) for k in range(PER_FRAME)]
            Q = len(groups)
            mqd = torch.tensor(mq, dtype=torch.int32, device=pid.device)
            run = {"kernel": lambda: DE.depth_residuals(depth, pid, sensor, mqd, Q, unit=UNIT, bin_m=BIN_M, bins=BINS),
                   "torch": lambda: torch_hist(depth, pid, sensor, groups)}
            calls = {"kernel": args.calls, "torch": args.torch_calls}
            k, t = run["kernel"](), run["torch"]()
            torch.cuda.synchronize()
            equal = bool(torch.equal(k["hist"].to(torch.int64), t))
            ms = {"kernel": [], "torch": []}
            for rd in range(args.warmup + args.rounds):
                for name in ("kernel", "torch"):
                    v = timed(run[name], calls[name])
                    if rd >= args.warmup:
                        ms[name].append(v)
            c = k["counts"].cpu().numpy()
            row = {"frames": N, "queries": Q, "per_frame": per, "hist_equal_torch": equal, "covered_pixels": int(c[:, 0].sum()),
                   "in_range_pixels": int(c[:, 5].sum()), "median_mm_mean": float(np.nanmean(k["stats"][:, 0].cpu().numpy()) * 1e3)}
            for name in ("kernel", "torch"):
                row[f"{name}_ms_per_call"] = round(float(np.median(ms[name])), 4)
                row[f"{name}_ms_min_max"] = [round(min(ms[name]), 4), round(max(ms[name]), 4)]
                row[f"{name}_calls_per_round"] = calls[name]
            row["torch_over_kernel"] = round(row["torch_ms_per_call"] / row["kernel_ms_per_call"], 2)
            row["pred_id_tb_per_s"] = round(N * H * W * 4 / (row["kernel_ms_per_call"] * 1e-3) / 1e12, 3)
            row["mask_boxes_tb_per_s"] = MASK_BOXES_TB_S.get(N)
            rows.append(row)
            lines.append(f"{N:3d} frames x {per} queries: hm_depth_residuals {row['kernel_ms_per_call']:.4f} ms "
                         f"[{row['kernel_ms_min_max'][0]:.4f}, {row['kernel_ms_min_max'][1]:.4f}] = {row['pred_id_tb_per_s']:.3f} TB/s of pred_id "
                         f"(hm_mask_boxes: {row['mask_boxes_tb_per_s']} TB/s of masks)  torch ops {row['torch_ms_per_call']:.3f} ms "
                         f"[{row['torch_ms_min_max'][0]:.3f}, {row['torch_ms_min_max'][1]:.3f}]  ({row['torch_over_kernel']}x)  "
                         f"covered {row['covered_pixels']}  hist equal: {equal}")
            print(lines[-1], file=sys.stderr)
            del run, k, t
        del depth, pid, sensor, r
        render.release_workspaces()
        DE.release_workspaces()
        torch.cuda.empty_cache()

    # (c) two iterations of refine_cam_t: the hands start 5 % nearer than the meshes the sensor saw
    N = args.refine_frames
    v, f = surface_mesh()
    faces = torch.from_numpy(f).cuda()
    rng = np.random.default_rng(0)
    B = N * PER_FRAME
    z = rng.uniform(0.5, 0.9, B)
    truth = np.stack([(rng.uniform(0.2, 0.8, B) * W - W / 2) * z / 1000.0, (rng.uniform(0.2, 0.8, B) * H - H / 2) * z / 1000.0, z], 1)
    verts = torch.from_numpy(np.repeat(v[None].astype(np.float32), B, 0)).cuda()
    frame_index = [j // PER_FRAME for j in range(B)]
    placed = verts + torch.from_numpy(truth.astype(np.float32)).cuda()[:, None, :]
    seen = render.render_views(H, W, K, [{"frame": frame_index[j], "vertices": placed[j], "faces": faces} for j in range(B)],
                               outputs=("depth",), views=N)["depth"]
    sensor = torch.round(torch.where(seen > 0, seen, torch.full_like(seen, 1.5)) / UNIT).to(torch.int32).to(torch.int16)
    start = torch.from_numpy((truth / 1.05).astype(np.float32)).cuda()
    refine = lambda: DE.refine_cam_t(H, W, K, verts, faces, start, frame_index, sensor, unit=UNIT, iterations=2)      # noqa: E731
    out = refine()
    torch.cuda.synchronize()
    err = (out["cam_t"][:, 2].double().cpu().numpy() - truth[:, 2]) * 1e3
    ms = [timed(refine, args.refine_calls) for _ in range(args.warmup + args.rounds)][args.warmup:]
    ref = {"frames": N, "hands": B, "iterations": 2, "ms_per_call": round(float(np.median(ms)), 3), "ms_min_max": [round(min(ms), 3), round(max(ms), 3)],
           "updated": int(out["updated"].sum()), "tz_error_mm_median_abs": round(float(np.median(np.abs(err))), 3),
           "tz_error_mm_max_abs": round(float(np.abs(err).max()), 3), "start_error_mm_median_abs": round(float(np.median(truth[:, 2] * (1 - 1 / 1.05)) * 1e3), 3)}
    lines.append(f"refine_cam_t, 2 iterations, {N} frames / {B} hands: {ref['ms_per_call']:.3f} ms [{ref['ms_min_max'][0]:.3f}, {ref['ms_min_max'][1]:.3f}]  "
                 f"updated {ref['updated']}  |tz error| median {ref['tz_error_mm_median_abs']} mm, max {ref['tz_error_mm_max_abs']} mm "
                 f"(start: median {ref['start_error_mm_median_abs']} mm)")
    print(lines[-1], file=sys.stderr)
    render.release_workspaces()
    DE.release_workspaces()
    lines.append(json.dumps({"bench": "depth_eval", "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "warmup": args.warmup,
                             "size": [H, W], "unit": UNIT, "bin_m": BIN_M, "bins": BINS, "rows": rows, "refine": ref}))
    print("\n".join(lines))
    if args.log:
        with open(args.log, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
