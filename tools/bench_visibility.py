"""hm_point_visibility and hm_mesh_coverage next to the hm_mesh_render call of the same scene.

  python tools/bench_visibility.py [--frames 16 64] [--rounds 6] [--warmup 2] [--calls 50] [--log profiles/visibility_bench.log]

Data: N frames of 1080 x 1920 with four hand-sized meshes each (tools/bench_render.py's ellipsoids: 780 vertices, 1500 faces),
rendered once by ``render_views``: its ``depth`` and ``mesh_id`` are the maps both calls read.  The sensor image is that depth
plus 10 mm in millimetres, a wall at 1.5 m where nothing is covered, shifted by (5, -7) pixels; the mask carries label 3 on
the covered pixels, shifted the other way.  The points are every mesh's vertices and 21 points inside it, two groups per mesh,
as ``hand_visibility`` makes them.

Timed, each through its Python wrapper with the meshes marked ``faces_checked`` (no read-back in the loop): (a)
``render_views`` with the depth and mesh_id outputs (hm_mesh_render), (b) ``point_visibility`` with the group table already on
the device, (c) ``mesh_coverage``; (b) and (c) with sensor and mask, and without.  A round is ``--calls`` back-to-back calls
between two device events; the three alternate round by round in one process after ``--warmup`` rounds of each; reported: the
median round as ms per call with the fastest and slowest round.  This is the time a call takes in a busy loop, host
submission included.  The parent commit's rate for the hm_mesh_render call of this scene was 0.96 ms at 16 frames and 3.24 ms
at 64 frames (tools/bench_render.py).  There is no pass mark.  One line per point and one JSON line go to stdout and to
``--log``.

Measured on an MI355X (profiles/visibility_bench.log, one run): 16 frames hm_mesh_render 0.688 ms, hm_point_visibility 0.042 ms
(0.045 ms with sensor and mask), hm_mesh_coverage 0.300 ms (0.286 ms); 64 frames 2.349 ms, 0.321 ms (0.321 ms), 1.050 ms
(1.047 ms).  The render's figure is below the parent's because the meshes are marked ``faces_checked`` here.  DESIGN.md
section 10.6."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

H, W, PER_FRAME, UNIT = 1080, 1920, 4, 0.001
PARENT_RENDER_MS = {16: 0.96, 64: 3.24}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="+", default=[16, 64])
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--log", type=str, default=os.path.join(ROOT, "profiles", "visibility_bench.log"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_visibility.py measures on the GPU; none is visible")
    from bench_render import _meshes
    from hamer_yolo_amd import render
    from hamer_yolo_amd.hamer.utils import visibility as V

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
        meshes = [dict(m, faces_checked=True) for m in _meshes(N, PER_FRAME)]
        r = render.render_views(H, W, K, meshes, outputs=("depth", "mesh_id"), views=N)
        depth, mid = r["depth"], r["mesh_id"]
        sensor = torch.round(torch.where(depth > 0, depth + 0.010, torch.full_like(depth, 1.5)) / UNIT).to(torch.int32).to(torch.int16)
        sensor = torch.roll(sensor, (5, -7), (1, 2)).contiguous()
        mask = torch.roll((mid >= 0).to(torch.uint8) * 3, (-4, 6), (1, 2)).contiguous()
        nv = int(meshes[0]["vertices"].shape[0])
        centres = torch.stack([m["vertices"].mean(0) for m in meshes])
        inner = torch.cat([c + 0.5 * (m["vertices"][::nv // 21][:21] - c) for m, c in zip(meshes, centres)])
        points = torch.cat([m["vertices"] for m in meshes] + [inner]).to(torch.float64).contiguous()
        B = len(meshes)
        groups = []
        for i, m in enumerate(meshes):
            groups.append(dict(view=m["frame"], mesh=i, p0=i * nv, np=nv, tol_m=V.VERTEX_TOL_M, label=3))
            groups.append(dict(view=m["frame"], mesh=i, p0=B * nv + 21 * i, np=21, tol_m=V.JOINT_TOL_M, label=3))
        gd = torch.from_numpy(V.pack_groups(groups)).to(depth.device)
        side = dict(sensor=sensor, unit=UNIT, mask=mask)
        labels = torch.full((B,), 3, dtype=torch.int32, device=depth.device)
        run = {"render": lambda: render.render_views(H, W, K, meshes, outputs=("depth", "mesh_id"), views=N),
               "points": lambda: V.point_visibility(depth, mid, K, points, gd, window=1),
               "points_side": lambda: V.point_visibility(depth, mid, K, points, gd, window=1, **side),
               "coverage": lambda: V.mesh_coverage(H, W, K, meshes, depth, mid),
               "coverage_side": lambda: V.mesh_coverage(H, W, K, meshes, depth, mid, labels=labels, **side)}
        first = {k: fn() for k, fn in run.items()}
        torch.cuda.synchronize()
        cx = first["coverage_side"][0].cpu().numpy()
        cp = first["points_side"][1].cpu().numpy()
        ok = bool((cx[:, 0] == cx[:, 1] + cx[:, 2] + cx[:, 7]).all() and (cx[:, 1] == cx[:, 3] + cx[:, 4] + cx[:, 6]).all()
                  and int(cx[:, 1].sum()) == int((mid >= 0).sum()) and (cp[:, :7].sum(1) == cp[:, 7]).all())
        ms = {k: [] for k in run}
        for rd in range(args.warmup + args.rounds):
            for name in run:
                v = timed(run[name], args.calls)
                if rd >= args.warmup:
                    ms[name].append(v)
        row = {"frames": N, "meshes": B, "points": int(points.shape[0]), "groups": len(groups), "amodal_pixels": int(cx[:, 0].sum()),
               "modal_pixels": int(cx[:, 1].sum()), "visible_vertices": int(cp[::2, 0].sum()), "identities_hold": ok,
               "parent_render_ms_per_call": PARENT_RENDER_MS.get(N)}
        for name in run:
            row[f"{name}_ms_per_call"] = round(float(np.median(ms[name])), 4)
            row[f"{name}_ms_min_max"] = [round(min(ms[name]), 4), round(max(ms[name]), 4)]
        rows.append(row)
        lines.append(f"{N:3d} frames x {PER_FRAME} meshes: hm_mesh_render {row['render_ms_per_call']:.4f} ms "
                     f"[{row['render_ms_min_max'][0]:.4f}, {row['render_ms_min_max'][1]:.4f}] (parent: {row['parent_render_ms_per_call']} ms)  "
                     f"hm_point_visibility {row['points_ms_per_call']:.4f} ms, with sensor and mask {row['points_side_ms_per_call']:.4f} ms "
                     f"({row['points']} points)  hm_mesh_coverage {row['coverage_ms_per_call']:.4f} ms, with sensor and mask "
                     f"{row['coverage_side_ms_per_call']:.4f} ms ({row['amodal_pixels']} amodal pixels)  identities hold: {ok}")
        print(lines[-1], file=sys.stderr)
        del run, first, depth, mid, sensor, mask, r
        render.release_workspaces()
        V.release_workspaces()
        torch.cuda.empty_cache()
    lines.append(json.dumps({"bench": "visibility", "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "warmup": args.warmup,
                             "calls": args.calls, "size": [H, W], "rows": rows}))
    print("\n".join(lines))
    if args.log:
        with open(args.log, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
