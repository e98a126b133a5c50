"""hm_track_smooth and hm_track_jitter next to the same quantities computed with torch ops on the device, and smooth_folder end
to end.

  python tools/bench_motion.py [--frames 64 1024 16384] [--radii 4 32] [--points 21 778] [--records 1024]
                               [--rounds 6] [--warmup 2] [--calls 20] [--log profiles/motion_bench.log]

Data: S = 2 tracks of J = 16 rotations and C = 13 channels, a seeded smooth motion plus noise, one hand in ten absent.
  * ``track_smooth`` (one hm_track_smooth launch) against the TORCH ROUTE: the sequence padded by R absent frames, ``unfold`` into
    windows of 2 R + 1, the pair mask from the presence windows, one weighted sum (einsum), a division, and ``torch.linalg.svd``
    for the nearest rotation.  Reported with it: the largest element difference between the two over the SMOOTHED and FILLED
    hands (the torch route sums in another order and projects by SVD), not asserted.
  * ``track_jitter`` (one hm_track_jitter launch) at N = the largest ``--frames`` against three slices, a norm and a mean in torch.
  * ``evaluate_motion.smooth_folder`` on ``--records`` synthetic records in a temporary folder, wall time, files included.

Each device quantity is timed through its Python wrapper: a round is ``--calls`` back-to-back calls between two device events;
kernel and torch route alternate round by round in one process after ``--warmup`` rounds of each; reported: the median round as
ms per call with the fastest and slowest round.  Next to it the DEVICE time of the kernel alone (``lib.profile``: the launch
between two events), the median of ``--calls`` calls.  There is no pass mark: the parent commit has no such call.  One line per
point and one JSON line go to stdout and to ``--log``."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="+", default=[64, 1024, 16384])
    ap.add_argument("--radii", type=int, nargs="+", default=[4, 32])
    ap.add_argument("--points", type=int, nargs="+", default=[21, 778])
    ap.add_argument("--records", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--log", type=str, default=os.path.join(ROOT, "profiles", "motion_bench.log"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_motion.py measures on the GPU; none is visible")
    from test_motion_host import rotmat
    from hamer_yolo_amd import lib as L
    from hamer_yolo_amd.hamer.utils import motion as MO
    dev = torch.device("cuda", 0)
    S, J, C = 2, 16, 13

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

    def alternate(run):
        ms = {k: [] for k in run}
        for rd in range(args.warmup + args.rounds):
            for name in run:
                t = timed(run[name], args.calls)
                if rd >= args.warmup:
                    ms[name].append(t)
        return {k: (round(float(np.median(v)), 4), round(min(v), 4), round(max(v), 4)) for k, v in ms.items()}

    def sequence(N, seed):
        rng = np.random.default_rng(seed)
        t = np.arange(N, dtype=np.float64)[:, None, None, None]
        aa = rng.normal(size=(1, S, J, 3)) * 0.3 + 0.3 * np.sin(t / 20.0 + rng.uniform(0, 6, size=(1, S, J, 3))) + \
            rng.normal(size=(N, S, J, 3)) * np.radians(3.0)
        lin = np.sin(t[:, :, :, 0] / 15.0) * 0.1 + rng.normal(size=(N, S, C)) * 0.003
        present = (rng.uniform(size=(N, S)) < 0.9).astype(np.uint8)
        return (torch.from_numpy(rotmat(aa)).to(dev), torch.from_numpy(lin).to(dev), torch.from_numpy(present).to(dev), aa, lin, present)

    def torch_smooth(rot, lin, present, w):
        R = len(w) - 1
        N = rot.shape[0]
        here = present.to(torch.float64)
        x = torch.cat([rot.reshape(N, S, J * 9), lin], 2) * here[:, :, None]
        pad = lambda a: torch.nn.functional.pad(a, (0,) * (2 * (a.dim() - 1)) + (R, R))   # noqa: E731
        xw = pad(x).unfold(0, 2 * R + 1, 1)                               # (N, S, J 9 + C, 2 R + 1)
        hw = pad(here).unfold(0, 2 * R + 1, 1)                            # (N, S, 2 R + 1)
        k = torch.arange(2 * R + 1, device=dev)
        use = hw * hw.flip(2)                                             # both ends of a pair; the centre with itself
        wk = w[(k - R).abs()] * use
        W = wk.sum(2)
        mean = torch.einsum("nsck,nsk->nsc", xw, wk) / W[:, :, None]
        m = mean[:, :, :J * 9].reshape(N, S, J, 3, 3)
        ok = (use.sum(2) - use[:, :, R]) > 0
        u, _, vt = torch.linalg.svd(torch.where(ok[:, :, None, None, None], m, torch.eye(3, dtype=torch.float64, device=dev)))
        return u @ vt, mean[:, :, J * 9:], ok

    lines, rows = [], []
    for N in args.frames:
        rot, lin, present, _, _, _ = sequence(N, N)
        for R in args.radii:
            w = torch.from_numpy(MO.window_weights(R, 2.0)).to(dev)
            run = {"kernel": lambda: MO.track_smooth(rot, lin, present, R, 2.0), "torch": lambda: torch_smooth(rot, lin, present, w)}
            got, (tr, tl, _) = run["kernel"](), run["torch"]()
            torch.cuda.synchronize()
            filt = (got["status"] == MO.SMOOTHED) | (got["status"] == MO.FILLED)
            diff = max(float((got["rot"] - tr)[filt].abs().max()), float((got["lin"] - tl)[filt].abs().max())) if bool(filt.any()) else 0.0
            ms = alternate(run)
            row = {"what": "track_smooth", "frames": N, "radius": R, "kernel_ms_per_call": ms["kernel"][0], "kernel_ms_min_max": ms["kernel"][1:],
                   "torch_ms_per_call": ms["torch"][0], "torch_ms_min_max": ms["torch"][1:],
                   "kernel_device_ms": round(float(device_ms(run["kernel"], args.calls)), 4), "max_abs_difference": diff,
                   "degenerate": int((got["status"] == MO.DEGENERATE).sum()), "filtered": int(filt.sum())}
            rows.append(row)
            lines.append(f"track_smooth N={N:5d} R={R:2d}: kernel {row['kernel_ms_per_call']:.4f} ms [{ms['kernel'][1]:.4f}, {ms['kernel'][2]:.4f}], on the device "
                         f"{row['kernel_device_ms']:.4f} ms; torch route {row['torch_ms_per_call']:.4f} ms [{ms['torch'][1]:.4f}, {ms['torch'][2]:.4f}]; "
                         f"largest difference {diff:.3g} over {row['filtered']} hands, {row['degenerate']} degenerate")
            print(lines[-1], file=sys.stderr)
    N = max(args.frames)
    for P in args.points:
        rng = np.random.default_rng(P)
        x = torch.from_numpy(np.cumsum(rng.normal(size=(N, S, P, 3)) * 0.002, axis=0)).to(dev)
        present = torch.from_numpy((rng.uniform(size=(N, S)) < 0.9).astype(np.uint8)).to(dev)

        def torch_jitter():
            d = (x[:-2] - 2.0 * x[1:-1]) + x[2:]
            a = torch.linalg.vector_norm(d, dim=3).mean(2)
            ok = (present[:-2] & present[1:-1] & present[2:]) != 0
            return torch.where(ok, a, torch.full_like(a, float("nan")))
        run = {"kernel": lambda: MO.track_jitter(x, present), "torch": torch_jitter}
        a, b = run["kernel"]()[1:-1], run["torch"]()
        torch.cuda.synchronize()
        diff = float((a - b)[torch.isfinite(b)].abs().max())
        ms = alternate(run)
        row = {"what": "track_jitter", "frames": N, "points": P, "kernel_ms_per_call": ms["kernel"][0], "kernel_ms_min_max": ms["kernel"][1:],
               "torch_ms_per_call": ms["torch"][0], "torch_ms_min_max": ms["torch"][1:],
               "kernel_device_ms": round(float(device_ms(run["kernel"], args.calls)), 4), "max_abs_difference": diff}
        rows.append(row)
        lines.append(f"track_jitter N={N:5d} P={P:4d}: kernel {row['kernel_ms_per_call']:.4f} ms [{ms['kernel'][1]:.4f}, {ms['kernel'][2]:.4f}], on the device "
                     f"{row['kernel_device_ms']:.4f} ms; torch route {row['torch_ms_per_call']:.4f} ms [{ms['torch'][1]:.4f}, {ms['torch'][2]:.4f}]; "
                     f"largest difference {diff:.3g}")
        print(lines[-1], file=sys.stderr)
    if args.records > 0:
        from hamer_yolo_amd import evaluate_motion as EM

        class _Device:
            device = dev
        _, _, _, aa, lin, present = sequence(args.records, 7)
        with tempfile.TemporaryDirectory() as tmp:
            src, out = os.path.join(tmp, "in"), os.path.join(tmp, "out")
            os.makedirs(src)
            for t in range(args.records):
                rec = {}
                for s, side in enumerate(MO.SIDES):
                    a = aa[t, s].astype(np.float32)
                    rec[side] = {"betas": lin[t, s, 3:].astype(np.float32), "theta": a.reshape(-1), "pose_hand": a[1:].reshape(-1),
                                 "pose_global": a[0].copy(), "cam_t": lin[t, s, :3].astype(np.float32), "is_right": s == 0} if present[t, s] else None
                np.save(os.path.join(src, f"f_{t}.npy"), rec)
            EM.smooth_folder(src, out, _Device())                          # warm: the files are in the page cache, the kernel is loaded
            walls = []
            for _ in range(3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                res = EM.smooth_folder(src, out, _Device())
                walls.append((time.perf_counter() - t0) * 1e3)
        row = {"what": "smooth_folder", "records": args.records, "wall_ms": round(float(np.median(walls)), 2), "wall_ms_min_max": [round(min(walls), 2), round(max(walls), 2)],
               **{k: res[k] for k in ("smoothed", "filled", "kept", "degenerate")}}
        rows.append(row)
        lines.append(f"smooth_folder on {args.records} records: {row['wall_ms']:.2f} ms wall [{row['wall_ms_min_max'][0]:.2f}, {row['wall_ms_min_max'][1]:.2f}] "
                     f"({row['wall_ms'] / args.records:.3f} ms per record; {res['smoothed']} hands smoothed, {res['filled']} filled, {res['kept']} kept)")
        print(lines[-1], file=sys.stderr)
    lines.append(json.dumps({"bench": "motion", "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "warmup": args.warmup,
                             "calls": args.calls, "rows": rows}))
    print("\n".join(lines))
    if args.log:
        os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
        with open(args.log, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
