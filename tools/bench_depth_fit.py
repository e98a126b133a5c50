"""hm_depth_fit against the same sums from torch ops on the same device tensors, against hm_depth_residuals at the same shape
(the one-pass yardstick of profiles/depth_eval_bench.log), and six rigid rounds of fit_rigid.

  python tools/bench_depth_fit.py [--frames 16 64] [--rounds 10] [--warmup 3] [--log profiles/depth_fit_bench.log]

Data: N frames of 1080 x 1920 with four hand-sized meshes each (tools/bench_render.py's ellipsoids), rendered once by
``render_views``: its ``depth`` and ``mesh_id`` are the prediction, one query per mesh, the pivot of a query the centre of its
mesh.  The sensor image is that depth plus 10 mm in millimetres, a wall at 1.5 m where nothing is covered, shifted by (5, -7)
pixels so that the footprints do not agree.

(a) one ``depth_fit`` call (three kernels); (b) ``torch_sums``: the rule in torch ops, fp64, one pass over all pixels and an
``index_add_`` per output; (c) one ``depth_residuals`` call on the same maps and queries; (d) ``fit_rigid`` with six rigid rounds
and no ray round over 64 frames' 256 hands, which start 3 degrees and (3, -2, 4) mm off.

A round is ``--calls`` back-to-back calls between two device events ((b): ``--torch-calls``, (d): ``--rigid-calls``); (a), (b)
and (c) alternate round by round in one process after ``--warmup`` rounds; reported: the median round as ms per call with the
fastest and slowest round, whether the two sides' sums and counts are equal, and the pixels used.  This is the time a call takes
in a busy loop, host submission included.  One line per point and one JSON line go to stdout and to ``--log``."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

H, W, PER_FRAME, UNIT = 1080, 1920, 4, 0.001
KW = dict(gate_m=0.03, edge_m=0.005, reach_m=0.5, damping=1e-3, lever_m=0.05, min_pixels=200)


def torch_sums(depth, pid, sensor, cams, pivot, Q):
    """(sums (Q, 28), counts (Q, 8)) int64 on the device by torch ops alone, one query per mesh id; the rule's order in fp64."""
    import torch
    import torch.nn.functional as F
    N = pid.shape[0]
    f64 = torch.float64
    d = depth.to(f64)
    raw = sensor.to(torch.int32) & 0xFFFF
    q = pid.to(torch.int64)
    cov = (pid >= 0) & (pid < Q)
    counts = torch.zeros(Q, 8, dtype=torch.int64, device=pid.device)

    def count(col, sel):
        counts[:, col] += torch.bincount(q[sel], minlength=Q)

    count(0, cov)
    none = cov & (raw == 0)
    count(2, none)
    ok = cov & ~none
    rz = raw.to(f64) * UNIT - d
    gated = ok & ~(rz.abs() <= KW["gate_m"])
    count(3, gated)
    ok = ok & ~gated

    def shifted(t, dv, du, fill):
        return F.pad(t, (1, 1, 1, 1), value=fill)[:, 1 + dv:1 + dv + H, 1 + du:1 + du + W]

    good = torch.ones_like(ok)
    nb = {}
    for name, dv, du in (("l", 0, -1), ("r", 0, 1), ("u", -1, 0), ("d", 1, 0)):
        nb[name] = shifted(d, dv, du, float("nan"))
        good &= (shifted(pid, dv, du, -2) == pid) & ((nb[name] - d).abs() <= KW["edge_m"])
    count(4, ok & ~good)
    ok = ok & good
    u = torch.arange(W, device=pid.device, dtype=f64)[None, None, :]
    v = torch.arange(H, device=pid.device, dtype=f64)[None, :, None]
    fx, fy, cx, cy = (cams[:, k][:, None, None] for k in range(4))
    rx, rxl, rxr = (u - cx) / fx, ((u - 1.0) - cx) / fx, ((u + 1.0) - cx) / fx
    ry, ryu, ryd = (v - cy) / fy, ((v - 1.0) - cy) / fy, ((v + 1.0) - cy) / fy
    ax, ay, az = nb["r"] * rxr - nb["l"] * rxl, nb["r"] * ry - nb["l"] * ry, nb["r"] - nb["l"]
    bx, by, bz = nb["d"] * rx - nb["u"] * rx, nb["d"] * ryd - nb["u"] * ryu, nb["d"] - nb["u"]
    nx, ny, nz = ay * bz - az * by, az * bx - ax * bz, ax * by - ay * bx
    l2 = nx * nx + ny * ny + nz * nz
    pv = pivot[q.clamp(0, Q - 1)]
    mx, my, mz = d * rx - pv[..., 0], d * ry - pv[..., 1], d - pv[..., 2]
    rho = (nx * rx + ny * ry + nz) * rz
    mm = mx * mx + my * my + mz * mz
    rej = ~((l2 > 0.0) & (l2 <= torch.finfo(f64).max)) | (mm > KW["reach_m"] * KW["reach_m"]) | (rho * rho > l2)
    count(5, ok & rej)
    use = ok & ~rej
    count(6, use)
    J = [my * nz - mz * ny, mz * nx - mx * nz, mx * ny - my * nx, nx, ny, nz]
    qs, l2u = q[use], l2[use]
    Ju, rhou = [j[use] for j in J], rho[use]
    sums = torch.zeros(Q, 28, dtype=torch.int64, device=pid.device)
    terms = [(Ju[i] * Ju[j]) for i in range(6) for j in range(i, 6)] + [Ju[i] * rhou for i in range(6)] + [rhou * rhou]
    for k, t in enumerate(terms):
        sums[:, k].index_add_(0, qs, torch.round(t / l2u * 2.0 ** 30).to(torch.int64))
    return sums, counts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="+", default=[16, 64])
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--torch-calls", type=int, default=2)
    ap.add_argument("--rigid-calls", type=int, default=2)
    ap.add_argument("--rigid-frames", type=int, default=64)
    ap.add_argument("--log", type=str, default=os.path.join(ROOT, "profiles", "depth_fit_bench.log"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_depth_fit.py measures on the GPU; none is visible")
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
        meshes = _meshes(N, PER_FRAME)
        r = render.render_views(H, W, K, meshes, outputs=("depth", "mesh_id"), views=N)
        depth, pid = r["depth"], r["mesh_id"]
        sensor = sensor_of(depth)
        Q = N * PER_FRAME
        pivot = torch.stack([torch.as_tensor(m["vertices"]).to(depth.device, torch.float64).reshape(-1, 3).mean(0) for m in meshes]).contiguous()
        cams = DE._cameras(K, N, depth.device)
        Kn = torch.from_numpy(np.repeat(K[None], N, 0)).to(depth.device)
        mqd = torch.arange(Q, dtype=torch.int32, device=pid.device)
        torch.cuda.synchronize()
        run = {"fit": lambda: DE.depth_fit(depth, pid, sensor, mqd, Q, Kn, pivot, unit=UNIT, **KW),
               "torch": lambda: torch_sums(depth, pid, sensor, cams, pivot, Q),
               "residuals": lambda: DE.depth_residuals(depth, pid, sensor, mqd, Q, unit=UNIT)}
        calls = {"fit": args.calls, "torch": args.torch_calls, "residuals": args.calls}
        k, t = run["fit"](), run["torch"]()
        torch.cuda.synchronize()
        equal = bool(torch.equal(k["sums"], t[0]) and torch.equal(k["counts"], t[1]))
        ms = {name: [] for name in run}
        for rd in range(args.warmup + args.rounds):
            for name in run:
                val = timed(run[name], calls[name])
                if rd >= args.warmup:
                    ms[name].append(val)
        c = k["counts"].cpu().numpy()
        row = {"frames": N, "queries": Q, "equal_torch": equal, "covered_pixels": int(c[:, 0].sum()), "used_pixels": int(c[:, 6].sum()),
               "no_normal_pixels": int(c[:, 4].sum()), "solved": int(k["solution"][:, 7].sum().item())}
        for name in run:
            row[f"{name}_ms_per_call"] = round(float(np.median(ms[name])), 4)
            row[f"{name}_ms_min_max"] = [round(min(ms[name]), 4), round(max(ms[name]), 4)]
            row[f"{name}_calls_per_round"] = calls[name]
        row["torch_over_fit"] = round(row["torch_ms_per_call"] / row["fit_ms_per_call"], 2)
        row["fit_over_residuals"] = round(row["fit_ms_per_call"] / row["residuals_ms_per_call"], 2)
        row["pred_id_tb_per_s"] = round(N * H * W * 4 / (row["fit_ms_per_call"] * 1e-3) / 1e12, 3)
        row["used_gpixels_per_s"] = round(row["used_pixels"] / (row["fit_ms_per_call"] * 1e-3) / 1e9, 3)
        rows.append(row)
        lines.append(f"{N:3d} frames x {PER_FRAME} queries: hm_depth_fit {row['fit_ms_per_call']:.4f} ms "
                     f"[{row['fit_ms_min_max'][0]:.4f}, {row['fit_ms_min_max'][1]:.4f}] = {row['pred_id_tb_per_s']:.3f} TB/s of pred_id, "
                     f"{row['used_gpixels_per_s']:.3f} G used pixels/s  hm_depth_residuals {row['residuals_ms_per_call']:.4f} ms "
                     f"({row['fit_over_residuals']}x)  torch ops {row['torch_ms_per_call']:.3f} ms "
                     f"[{row['torch_ms_min_max'][0]:.3f}, {row['torch_ms_min_max'][1]:.3f}]  ({row['torch_over_fit']}x)  "
                     f"covered {row['covered_pixels']} used {row['used_pixels']}  sums and counts equal: {equal}")
        print(lines[-1], file=sys.stderr)
        del run, k, t, depth, pid, sensor, r
        render.release_workspaces()
        DE.release_workspaces()
        DE.release_fit_workspaces()
        torch.cuda.empty_cache()

    # (d) six rigid rounds: the hands start 3 degrees and (3, -2, 4) mm from the meshes the sensor saw
    N = args.rigid_frames
    v, f = surface_mesh()
    faces = torch.from_numpy(f).cuda()
    rng = np.random.default_rng(0)
    B = N * PER_FRAME
    z = rng.uniform(0.5, 0.9, B)
    truth = np.stack([(rng.uniform(0.2, 0.8, B) * W - W / 2) * z / 1000.0, (rng.uniform(0.2, 0.8, B) * H - H / 2) * z / 1000.0, z], 1)
    frame_index = [j // PER_FRAME for j in range(B)]
    true_placed = torch.from_numpy(v[None] + truth[:, None, :]).cuda()
    seen = render.render_views(H, W, K, [{"frame": frame_index[j], "vertices": true_placed[j], "faces": faces} for j in range(B)],
                               outputs=("depth",), views=N)["depth"]
    sensor = torch.round(torch.where(seen > 0, seen, torch.full_like(seen, 1.5)) / UNIT).to(torch.int32).to(torch.int16)
    axes = rng.normal(size=(B, 3))
    w = torch.from_numpy(axes / np.linalg.norm(axes, axis=1, keepdims=True) * np.radians(3.0)).cuda()
    verts = torch.einsum("bij,vj->bvi", DE.exp_so3(w), torch.from_numpy(v).cuda()).to(torch.float32)
    start = torch.from_numpy((truth + np.array([0.003, -0.002, 0.004])).astype(np.float32)).cuda()
    rigid = lambda: DE.fit_rigid(H, W, K, verts, faces, start, start.to(torch.float64), frame_index, sensor, unit=UNIT,      # noqa: E731
                                 ray_iterations=0, iterations=6)
    out = rigid()
    torch.cuda.synchronize()
    e0 = (verts.double() + start.double()[:, None, :] - true_placed).norm(dim=2).mean(1).cpu().numpy() * 1e3
    e1 = (out["placed"] - true_placed).norm(dim=2).mean(1).cpu().numpy() * 1e3
    ms = [timed(rigid, args.rigid_calls) for _ in range(args.warmup + args.rounds)][args.warmup:]
    rig = {"frames": N, "hands": B, "iterations": 6, "ms_per_call": round(float(np.median(ms)), 3), "ms_min_max": [round(min(ms), 3), round(max(ms), 3)],
           "fitted": int(out["fitted"].sum()), "start_error_mm_median": round(float(np.median(e0)), 3),
           "end_error_mm_median": round(float(np.median(e1)), 3), "end_error_mm_max": round(float(e1.max()), 3)}
    lines.append(f"fit_rigid, 6 rigid rounds, {N} frames / {B} hands: {rig['ms_per_call']:.3f} ms [{rig['ms_min_max'][0]:.3f}, {rig['ms_min_max'][1]:.3f}]  "
                 f"fitted {rig['fitted']}  mean vertex error median {rig['end_error_mm_median']} mm, max {rig['end_error_mm_max']} mm "
                 f"(start: median {rig['start_error_mm_median']} mm)")
    print(lines[-1], file=sys.stderr)
    render.release_workspaces()
    DE.release_fit_workspaces()
    lines.append(json.dumps({"bench": "depth_fit", "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "warmup": args.warmup,
                             "size": [H, W], "unit": UNIT, **KW, "rows": rows, "rigid": rig}))
    print("\n".join(lines))
    if args.log:
        with open(args.log, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
