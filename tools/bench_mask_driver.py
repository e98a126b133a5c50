"""hm_mask_boxes and the batched mask-driven folder driver, measured ("The mask-driven folder driver").

  python tools/bench_mask_driver.py [--frames 16 64] [--per-frame 1 2] [--rounds 10] [--warmup 3]
                                    [--folder-frames 64] [--folder-rounds 5] [--log profiles/mask_boxes_bench.log]

Device part.  N label masks of 1080 x 1920 with two hand-sized blobs each (labels 3 and 4); one query per frame (label 3) or two
(3 and 4).  (a) one ``mask_boxes`` call with the query table already on the device: the two kernels; (b) ``torch_boxes``: the
same rows from torch ops on the same device tensor (a comparison per query, ``any`` along each axis, ``argmax`` of the two
profiles and their reverses, a sum); (c) the numpy rule on the host (``np.where`` per query, what ``get_bbox_from_npy`` does once
the file is loaded), timed with the host clock over ``--host-calls`` calls.  A round of (a) / (b) is ``--calls`` / ``--torch-calls``
back-to-back calls between two device events; (a) and (b) alternate round by round after ``--warmup`` rounds of both; reported:
the median round as ms per call with the fastest and slowest round, whether the three sides' rows are equal, and the frames'
bytes per second of (a) -- N H W bytes over the call time, host submission included; with two queries per frame the kernel
reads every frame twice -- against the 6.29 TB/s a device copy reaches.

End to end.  A folder of ``--folder-frames`` synthetic 1080 x 1920 BMP frames with one mask each (one hand per frame, label 3):
frames per second of ``process_batch_manopara_with_mask(batched=True)`` against the loop (``batched=False``) in the same
process, alternated round by round after one warm-up round of both, each round timed with the host clock around the whole call
(files written included); next to them ``process_batch_manopara`` over the same frames with the same boxes handed in by a
stand-in detector, for the pipeline's own cost at one hand per frame.  One more batched run with ``HAMER_E2E_TRACE=1`` puts the
host timeline of the pass into the log.  One line per point and one JSON line go to stdout and to ``--log``."""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

H, W = 1080, 1920
COPY_TBS = 6.29


def hand_mask(n: int) -> np.ndarray:
    """(H, W) uint8: a blob of label 3 and one of label 4, each the size of a hand at 1080p, placed by the frame's number."""
    yy, xx = np.mgrid[0:H, 0:W]
    m = np.zeros((H, W), np.uint8)
    cy, cx = 300 + (n * 37) % 500, 400 + (n * 101) % 1100
    m[((yy - cy) / 110.0) ** 2 + ((xx - cx) / 90.0) ** 2 < 1.0] = 3
    m[((yy - (H - cy)) / 100.0) ** 2 + ((xx - (W - cx)) / 95.0) ** 2 < 1.0] = 4
    return m


def torch_boxes(mask, frames, labels):
    """(Q, 5) int32 on the device by torch ops alone; ``frames`` / ``labels``: (Q,) int64 device tensors."""
    import torch
    eq = mask[frames] == labels[:, None, None].to(torch.uint8)
    cols, rows = eq.any(1), eq.any(2)
    n = eq.sum((1, 2), dtype=torch.int64)
    x1, y1 = cols.int().argmax(1), rows.int().argmax(1)
    x2 = cols.shape[1] - 1 - cols.flip(1).int().argmax(1)
    y2 = rows.shape[1] - 1 - rows.flip(1).int().argmax(1)
    box = torch.stack([x1, y1, x2, y2], 1)
    return torch.cat([torch.where((n > 0)[:, None], box, torch.full_like(box, -1)), n[:, None]], 1).to(torch.int32)


class GivenBoxes:
    """A detector stand-in that hands the pipeline the masks' boxes (one hand per frame) without looking at a pixel."""

    def __init__(self, boxes):
        self.boxes = boxes

    def detect_frames(self, frames):
        got, self.boxes = self.boxes[:len(frames)], self.boxes[len(frames):] + self.boxes[:len(frames)]
        return None, [[["right", b]] for b in got]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="+", default=[16, 64])
    ap.add_argument("--per-frame", type=int, nargs="+", default=[1, 2])
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--torch-calls", type=int, default=5)
    ap.add_argument("--host-calls", type=int, default=2)
    ap.add_argument("--folder-frames", type=int, default=64)
    ap.add_argument("--folder-rounds", type=int, default=5)
    ap.add_argument("--ckpt", type=str, default="synthetic:0")
    ap.add_argument("--log", type=str, default=os.path.join(ROOT, "profiles", "mask_boxes_bench.log"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_mask_driver.py measures on the GPU; none is visible")
    import mask_boxes_rule as BR
    from hamer_yolo_amd import infer, synth
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
    for N in args.frames:
        host = np.stack([hand_mask(n) for n in range(N)])
        mask = torch.from_numpy(host).cuda()
        for per in args.per_frame:
            queries = [(n, label) for n in range(N) for label in (3, 4)[:per]]
            qd = torch.tensor(queries, dtype=torch.int32, device="cuda")
            fr, lab = qd[:, 0].long(), qd[:, 1].long()
            out = torch.empty(len(queries), 5, dtype=torch.int32, device="cuda")
            run = {"kernel": lambda: ME.mask_boxes(mask, qd, boxes=out), "torch": lambda: torch_boxes(mask, fr, lab)}
            calls = {"kernel": args.calls, "torch": args.torch_calls}
            k, t = run["kernel"]().clone(), run["torch"]()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.host_calls):
                want = BR.boxes(host, queries)
            host_ms = (time.perf_counter() - t0) * 1e3 / args.host_calls
            equal = bool(torch.equal(k, t)) and bool(np.array_equal(k.cpu().numpy(), want))
            ms = {"kernel": [], "torch": []}
            for r in range(args.warmup + args.rounds):
                for name in ("kernel", "torch"):
                    v = timed(run[name], calls[name])
                    if r >= args.warmup:
                        ms[name].append(v)
            row = {"frames": N, "queries": len(queries), "per_frame": per, "rows_equal": equal, "numpy_rule_ms_per_call": round(host_ms, 3),
                   "numpy_rule_calls": args.host_calls}
            for name in ("kernel", "torch"):
                row[f"{name}_ms_per_call"] = round(float(np.median(ms[name])), 4)
                row[f"{name}_ms_min_max"] = [round(min(ms[name]), 4), round(max(ms[name]), 4)]
                row[f"{name}_calls_per_round"] = calls[name]
            row["frame_tb_per_s"] = round(N * H * W / (row["kernel_ms_per_call"] * 1e-3) / 1e12, 3)
            row["share_of_copy_rate"] = round(row["frame_tb_per_s"] / COPY_TBS, 3)
            rows.append(row)
            lines.append(f"{N:3d} frames x {per} queries: hm_mask_boxes {row['kernel_ms_per_call']:.4f} ms "
                         f"[{row['kernel_ms_min_max'][0]:.4f}, {row['kernel_ms_min_max'][1]:.4f}] = {row['frame_tb_per_s']:.3f} TB/s of frames "
                         f"({100 * row['share_of_copy_rate']:.1f} % of {COPY_TBS})  torch ops {row['torch_ms_per_call']:.3f} ms "
                         f"[{row['torch_ms_min_max'][0]:.3f}, {row['torch_ms_min_max'][1]:.3f}]  numpy rule {host_ms:.1f} ms  rows equal: {equal}")
            print(lines[-1], file=sys.stderr)
            del run, k, t
        del mask
        torch.cuda.empty_cache()

    # ------------------------------------------------------------------ end to end
    e2e = None
    if args.folder_frames > 0:
        from hamer_yolo_amd.config.hamer_config import hamer_opt
        from PIL import Image
        hamer_opt.ckpt_path = args.ckpt
        hamer = infer.hamer_inference(hamer_opt)
        root = tempfile.mkdtemp(prefix="mask_driver_bench_")
        try:
            rgb, masks = os.path.join(root, "rgb"), os.path.join(root, "masks")
            os.makedirs(rgb); os.makedirs(masks)
            boxes, pictures = [], []
            for n in range(args.folder_frames):
                if n < 8:                                          # eight distinct frames, repeated: the pixels do not matter here
                    pictures.append(Image.fromarray(synth.frame_u8(H, W, seed=900 + n).numpy()[:, :, ::-1]))
                pictures[n % 8].save(os.path.join(rgb, f"f{n:04d}.bmp"))
                m = np.where(hand_mask(n) == 3, 3, 0).astype(np.uint8)
                np.save(os.path.join(masks, f"f{n:04d}.npy"), m)
                boxes.append([float(v) for v in BR.box(m, 3)[:4]])

            def once(which, trace=False):
                out = os.path.join(root, f"out_{which}")
                shutil.rmtree(out, ignore_errors=True)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                if which == "loop":
                    st = infer.process_batch_manopara_with_mask(rgb, masks, out, hamer=hamer)
                elif which == "batched":
                    st = infer.process_batch_manopara_with_mask(rgb, masks, out, hamer=hamer, batched=True)
                else:
                    st = infer.process_batch_manopara(rgb, out, None, hamer=hamer, detector=GivenBoxes(list(boxes)))
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                assert len(os.listdir(out)) == args.folder_frames, (which, len(os.listdir(out)))
                return dt, st

            names = ("batched", "loop", "given_boxes")
            secs = {k: [] for k in names}
            stats = {}
            for r in range(1 + args.folder_rounds):
                for name in names:
                    dt, st = once(name)
                    if r >= 1:
                        secs[name].append(dt)
                        stats[name] = st
            os.environ["HAMER_E2E_TRACE"] = "1"
            _, traced = once("batched")
            os.environ.pop("HAMER_E2E_TRACE")
            a = np.load(os.path.join(root, "out_batched", "f0000.npy"), allow_pickle=True).item()["right"]
            b = np.load(os.path.join(root, "out_loop", "f0000.npy"), allow_pickle=True).item()["right"]
            e2e = {"frames": args.folder_frames, "rounds": args.folder_rounds,
                   "max_abs_diff_first_record": float(max(np.abs(a[k] - b[k]).max() for k in ("betas", "theta", "cam_t"))),
                   "forward_sizes": stats["batched"]["forward_sizes"], "det_pass_sizes": stats["batched"]["det_pass_sizes"],
                   "trace_ms": traced.get("trace", [])}
            for name in names:
                fps = [args.folder_frames / s for s in secs[name]]
                e2e[f"{name}_frames_per_s"] = round(float(np.median(fps)), 1)
                e2e[f"{name}_frames_per_s_min_max"] = [round(min(fps), 1), round(max(fps), 1)]
            e2e["batched_over_loop"] = round(e2e["batched_frames_per_s"] / e2e["loop_frames_per_s"], 2)
            lines.append(f"folder of {args.folder_frames} frames 1080 x 1920, one hand each: batched {e2e['batched_frames_per_s']} frames/s "
                         f"{e2e['batched_frames_per_s_min_max']}  loop {e2e['loop_frames_per_s']} frames/s {e2e['loop_frames_per_s_min_max']}  "
                         f"({e2e['batched_over_loop']}x)  process_batch_manopara with the boxes given {e2e['given_boxes_frames_per_s']} frames/s "
                         f"{e2e['given_boxes_frames_per_s_min_max']}  forwards {e2e['forward_sizes']}  passes {e2e['det_pass_sizes']}")
            lines.append("host timeline of one batched run (ms): " + "  ".join(f"{t}:{what}" for t, what in e2e["trace_ms"]))
            print("\n".join(lines[-2:]), file=sys.stderr)
        finally:
            shutil.rmtree(root, ignore_errors=True)
    lines.append(json.dumps({"bench": "mask_boxes", "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "warmup": args.warmup,
                             "size": [H, W], "rows": rows, "end_to_end": e2e}))
    print("\n".join(lines))
    if args.log:
        with open(args.log, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
