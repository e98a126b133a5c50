"""hm_mask_fit against the same sums from torch ops on the same device tensors, against hm_mask_score on the same maps, and six
rounds of fit_contour.

  python tools/bench_mask_fit.py [--frames 16 64] [--per-frame 1 4] [--rounds 10] [--warmup 3] [--log profiles/mask_fit_bench.log]

Data: tools/bench_mask_eval.py's -- N frames of 1080 x 1920 with four hand-sized meshes each, rendered once by ``render_views``:
its ``mesh_id`` is the prediction; the mask is the same image shifted by (5, -7) pixels with label 1 + (mesh index mod 4).
Radius 36 (``fit_radius(1080, 1920)``), both directions, the frame's centre as every query's centre.  With one query per frame
the union of the frame's hands is fitted to any label (label -1); with four, each hand to its own label.

(a) one ``mask_fit`` call (four kernels; the query and centre tables are on the device already); (b) ``torch_sums``: the rule in
torch ops on whole images -- boundary maps by comparisons with replicated shifts; per map the nearest set pixel at or left of and
right of every pixel of every row by a cumulative maximum / minimum of column indices; then for every row offset dy in
ascending order the nearer of the two within the chord, kept when its d2 is strictly less than the best so far (which is the
rule's order of preference); the terms in int64 and one fp64 division each -- queries in chunks of 4 to bound its memory;
(c) the ``mask_counts`` call (hm_mask_score, radius 18) on the same maps, for scale.  (d) ``fit_contour``: six rounds for
64 frames / 256 hands that start 2 % too far and (3, -2) mm off, every hand under its own label.

A round is ``--calls`` back-to-back calls between two device events ((b): ``--torch-calls``); (a) and (b) alternate round by
round in one process after ``--warmup`` rounds of both; reported: the median round as ms per call with the fastest and slowest
round, and whether the two sides' sums and counts are equal.  This is the time a call takes in a busy loop, host submission
included.  One line per point and one JSON line go to stdout and to ``--log``."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

H, W, RADIUS, SCORE_RADIUS, PER_FRAME, REACH = 1080, 1920, 36, 18, 4, 4096
BIG = 1 << 20


def torch_sums(pid, mask, queries, centre, r, directions=3, chunk=4):
    """(sums (Q, 18), counts (Q, 2, 6)) int64 on the device by torch ops alone."""
    import torch
    dev = pid.device
    Hh, Ww = int(pid.shape[1]), int(pid.shape[2])
    hw = [max(w for w in range(r + 1) if w * w + d * d <= r * r) for d in range(r + 1)]
    xs = torch.arange(Ww, device=dev, dtype=torch.int32)[None, None, :]
    ys = torch.arange(Hh, device=dev, dtype=torch.int32)[None, :, None]

    def bmap(s):
        e = torch.cat([s[:, :, 1:], s[:, :, -1:]], 2)
        so = torch.cat([s[:, 1:], s[:, -1:]], 1)
        se = torch.cat([so[:, :, 1:], so[:, :, -1:]], 2)
        return (s != e) | (s != so) | (s != se)

    def nearest(a, b):
        """Per pixel the rule's (dx, dy, d2) to the nearest set pixel of b (d2 = BIG: none)."""
        left = torch.cummax(torch.where(b, xs, -BIG), 2).values
        right = torch.flip(torch.cummin(torch.flip(torch.where(b, xs, BIG), (2,)), 2).values, (2,))
        left = torch.nn.functional.pad(left, (0, 0, r, r), value=-BIG)
        right = torch.nn.functional.pad(right, (0, 0, r, r), value=BIG)
        best = torch.full(a.shape, BIG, dtype=torch.int32, device=dev)
        bdx, bdy = torch.zeros_like(best), torch.zeros_like(best)
        for dy in range(-r, r + 1):
            w = hw[abs(dy)]
            dl, dr = xs - left[:, r + dy:r + dy + Hh], right[:, r + dy:r + dy + Hh] - xs             # both >= 0
            dx = torch.where(dl <= dr, -dl, dr)
            ad = torch.minimum(dl, dr)
            d2 = torch.where(ad <= w, ad * ad + dy * dy, BIG)
            take = a & (d2 < best)
            best = torch.where(take, d2, best)
            bdx = torch.where(take, dx, bdx)
            bdy = torch.where(take, torch.full_like(bdy, dy), bdy)
        return bdx, bdy, best

    sums, counts = [], []
    for i in range(0, len(queries), chunk):
        q = queries[i:i + chunk]
        f = torch.tensor([t[0] for t in q], device=dev)
        lo = torch.tensor([t[1] for t in q], device=dev, dtype=torch.int32)[:, None, None]
        hi = torch.tensor([t[2] for t in q], device=dev, dtype=torch.int32)[:, None, None]
        lab = torch.tensor([t[3] for t in q], device=dev, dtype=torch.int32)[:, None, None]
        cx = centre[i:i + chunk, 0].to(torch.int64)[:, None, None]
        cy = centre[i:i + chunk, 1].to(torch.int64)[:, None, None]
        p, m = pid[f], mask[f].to(torch.int32)
        bp, bg = bmap((p >= lo) & (p < hi)), bmap(torch.where(lab == -1, m != 0, m == lab))
        s = torch.zeros(len(q), 18, dtype=torch.int64, device=dev)
        c = torch.zeros(len(q), 2, 6, dtype=torch.int64, device=dev)
        for k, (a, b) in enumerate(((bp, bg), (bg, bp))):
            if not (directions >> k) & 1:
                continue
            dx, dy, d2 = nearest(a, b)
            dx, dy, d2 = dx.to(torch.int64), dy.to(torch.int64), d2.to(torch.int64)
            found = a & (d2 < BIG)
            if k == 0:
                ux, uy, ex, ey = xs - cx, ys - cy, dx, dy
            else:
                ux, uy, ex, ey = xs + dx - cx, ys + dy - cy, -dx, -dy
            reach = (ux.abs() <= REACH) & (uy.abs() <= REACH) & (ux * ux + uy * uy <= REACH * REACH)
            line, anchor = found & reach & (d2 > 0), found & reach & (d2 == 0)
            tot = lambda t: t.sum((1, 2), dtype=torch.int64)                                     # noqa: E731
            c[:, k, 0], c[:, k, 1], c[:, k, 2], c[:, k, 3], c[:, k, 4] = tot(a), tot(line), tot(anchor), tot(a & ~found), tot(found & ~reach)
            J = [ex * ux + ey * uy, ey * ux - ex * uy, ex + 0 * ux, ey + 0 * ux]
            den = torch.where(line, d2, torch.ones_like(d2)).to(torch.float64)
            n = 0
            for ii in range(4):
                for jj in range(ii, 4):
                    t = torch.round((J[ii] * J[jj]).to(torch.float64) / den * 1048576.0).to(torch.int64)
                    s[:, n] += tot(torch.where(line, t, torch.zeros_like(t)))
                    n += 1
            for ii in range(4):
                s[:, 10 + ii] += tot(torch.where(line, J[ii], torch.zeros_like(J[ii])))
            s[:, 14] += tot(torch.where(line, d2, torch.zeros_like(d2)))
            zero = torch.zeros_like(ux + 0 * d2)
            s[:, 15] += tot(torch.where(anchor, ux + 0 * d2, zero))
            s[:, 16] += tot(torch.where(anchor, uy + 0 * d2, zero))
            s[:, 17] += tot(torch.where(anchor, ux * ux + uy * uy, zero))
        sums.append(s)
        counts.append(c)
    return torch.cat(sums), torch.cat(counts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="+", default=[16, 64])
    ap.add_argument("--per-frame", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--torch-calls", type=int, default=1)
    ap.add_argument("--loop-frames", type=int, default=64)
    ap.add_argument("--log", type=str, default=os.path.join(ROOT, "profiles", "mask_fit_bench.log"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_mask_fit.py measures on the GPU; none is visible")
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

    def stats(v):
        return round(float(np.median(v)), 4), [round(min(v), 4), round(max(v), 4)]

    lines, rows = [], []
    K = np.array([[1000.0, 0, W / 2], [0, 1000.0, H / 2], [0, 0, 1]])
    dev = torch.device("cuda")
    for N in args.frames:
        meshes = _meshes(N, PER_FRAME)
        pid = render.render_views(H, W, K, meshes, outputs=("mesh_id",), views=N)["mesh_id"]
        shifted = torch.roll(pid, (5, -7), (1, 2))
        mask = torch.where(shifted >= 0, shifted % PER_FRAME + 1, torch.zeros_like(shifted)).to(torch.uint8)
        del shifted
        torch.cuda.synchronize()
        for per in args.per_frame:
            if per == 1:
                queries = [(n, n * PER_FRAME, (n + 1) * PER_FRAME, -1) for n in range(N)]
            else:
                queries = [(n, n * PER_FRAME + k, n * PER_FRAME + k + 1, k + 1) for n in range(N) for k in range(per)]
            qd = torch.tensor(queries, dtype=torch.int32, device=dev)
            cd = torch.tensor([(W // 2, H // 2)] * len(queries), dtype=torch.int32, device=dev)
            score_out = torch.empty(len(queries), 8, dtype=torch.int64, device=dev)
            run = {"fit": lambda: ME.mask_fit(pid, mask, qd, cd, radius=RADIUS, reach_px=REACH),
                   "torch": lambda: torch_sums(pid, mask, queries, cd, RADIUS),
                   "score": lambda: ME.mask_counts(pid, mask, queries, radius=SCORE_RADIUS, counts=score_out)}
            calls = {"fit": args.calls, "torch": args.torch_calls, "score": args.calls}
            k, t = run["fit"](), run["torch"]()
            torch.cuda.synchronize()
            equal = bool(torch.equal(k["sums"], t[0]) and torch.equal(k["counts"], t[1]))
            ms = {name: [] for name in run}
            for r in range(args.warmup + args.rounds):
                for name in run:
                    if name == "torch" and r >= args.warmup + 3:
                        continue                                                      # three rounds of the slow side are enough
                    v = timed(run[name], calls[name])
                    if r >= args.warmup:
                        ms[name].append(v)
            cnt = k["counts"].cpu().numpy()
            row = {"frames": N, "queries": len(queries), "per_frame": per, "radius": RADIUS, "sums_equal_torch": equal,
                   "boundary_pixels_per_query": float(cnt[:, :, 0].sum(1).mean()), "used_pixels_per_query": float(cnt[:, :, 1:3].sum((1, 2)).mean()),
                   "solved": int(k["solution"][:, 5].sum().item())}
            for name in run:
                row[f"{name}_ms_per_call"], row[f"{name}_ms_min_max"] = stats(ms[name])
            row["torch_over_fit"] = round(row["torch_ms_per_call"] / row["fit_ms_per_call"], 1)
            rows.append(row)
            lines.append(f"{N:3d} frames x {per} queries, r = {RADIUS}: hm_mask_fit {row['fit_ms_per_call']:.4f} ms "
                         f"[{row['fit_ms_min_max'][0]:.4f}, {row['fit_ms_min_max'][1]:.4f}]  torch ops {row['torch_ms_per_call']:.2f} ms "
                         f"({row['torch_over_fit']}x)  hm_mask_score (r = {SCORE_RADIUS}) {row['score_ms_per_call']:.4f} ms  "
                         f"{row['boundary_pixels_per_query']:.0f} boundary / {row['used_pixels_per_query']:.0f} used pixels per query  "
                         f"sums equal: {equal}")
            print(lines[-1], file=sys.stderr)
            del run, k, t
            torch.cuda.empty_cache()
        if N == args.loop_frames:
            # six rounds of fit_contour: every hand under its own label, started 2 % too far and (3, -2) mm off
            faces = meshes[0]["faces"]
            placed = torch.stack([m["vertices"] for m in meshes]).to(torch.float64)
            origin = placed.mean(1)
            verts = (placed - origin[:, None, :]).to(torch.float32)
            start = (origin * 1.02 + torch.tensor([0.003, -0.002, 0.0], dtype=torch.float64, device=dev)).to(torch.float32)
            frames = [m["frame"] for m in meshes]
            labels = [j % PER_FRAME + 1 for j in range(len(meshes))]
            truth = torch.where(pid >= 0, pid % PER_FRAME + 1, torch.zeros_like(pid)).to(torch.uint8)
            loop = lambda: ME.fit_contour(H, W, K, verts, faces, start, start.to(torch.float64), frames, truth, labels)      # noqa: E731
            out = loop()
            torch.cuda.synchronize()
            e0 = float(torch.linalg.norm(verts.to(torch.float64) + start[:, None, :].to(torch.float64) - placed, dim=2).mean()) * 1e3
            e1 = float(torch.linalg.norm(out["placed"] - placed, dim=2).mean()) * 1e3
            v = [timed(loop, 2) for _ in range(args.warmup + args.rounds)][args.warmup:]
            med, mm = stats(v)
            rows.append({"fit_contour_frames": N, "hands": len(meshes), "rounds": 6, "ms_per_call": med, "ms_min_max": mm,
                         "fitted": int(out["fitted"].sum().item()), "mean_vertex_error_mm": [round(e0, 3), round(e1, 3)],
                         "rms_px_mean": float(out["rms"].mean().item())})
            lines.append(f"fit_contour, {N} frames / {len(meshes)} hands, six rounds: {med:.2f} ms [{mm[0]:.2f}, {mm[1]:.2f}]; "
                         f"{rows[-1]['fitted']} fitted, mean vertex error {e0:.2f} -> {e1:.2f} mm")
            print(lines[-1], file=sys.stderr)
        del pid, mask, meshes
        render.release_workspaces()
        ME.release_workspaces()
        ME.release_fit_workspaces()
        torch.cuda.empty_cache()
    lines.append(json.dumps({"bench": "mask_fit", "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "warmup": args.warmup,
                             "size": [H, W], "rows": rows}))
    print("\n".join(lines))
    if args.log:
        with open(args.log, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
