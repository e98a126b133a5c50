"""NMS for a whole detector pass: the per-image loop (hm_yolo_nms, what the drivers call) against one hm_yolo_nms_batch call
(DESIGN.md section 11.1), on real passes of seeded 1080p frames through the synthetic detector (n = 15120 rows, 3 classes).

  python tools/bench_nms.py [--deployed-nb 16 48] [--test-nb 16 64] [--rounds 10] [--warmup 3] [--weights synthetic:2:-2.2:0]

Deployed thresholds (conf 0.25, IoU 0.35, best class, agnostic), per ``--deployed-nb``:
  loop_a, loop_b  YoloEngine.nms_enqueue as shipped: a memset and two launches per image (the same variant twice: its spread)
  batched         nms_enqueue(..., batched=True): a memset and two launches per pass
  The tool asserts that both leave the same ``dets`` / ``count`` bytes before it times anything.
test.py's protocol (conf 0.001, IoU 0.65, multi-label, class-aware), per ``--test-nb``:
  batch           one hm_yolo_nms_batch call for the pass
  serial          nb calls of the same entry with nb = 1, image after image: the work as a per-image design has to run it
  forward         the detector pass that produced ``pred`` (letterbox .. decode), for scale
  with the candidates per image (the kernel's own counters), how many images sorted in the workspace (> 16384 candidates)
  and how many were cut to 30000.
Every figure is the median over ``--rounds`` of the time between two device events around ``calls`` back-to-back enqueues,
after ``--warmup`` rounds, the variants alternating inside each round.  One JSON line per shape on stderr, one at the end."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--deployed-nb", type=int, nargs="+", default=[16, 48])
    ap.add_argument("--test-nb", type=int, nargs="+", default=[16, 64])
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--weights", type=str, default="synthetic:2:-2.2:0")
    args = ap.parse_args()
    import torch
    from hamer_yolo_amd import lib as L
    from hamer_yolo_amd import synth
    from hamer_yolo_amd.yolo.detector import Detector
    if not torch.cuda.is_available():
        raise SystemExit("bench_nms.py measures on the GPU; none is visible")

    class Cfg:
        weights = args.weights; imgsz = 640; augment = True; conf_thres = 0.25; iou_thres = 0.35
        classes = [0, 1, 2]; agnostic_nms = True; device = "cuda"; save_path = "./output"

    det = Detector(Cfg)
    eng, lib = det.engine, L.load()

    def dev_ms(fn, calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / calls

    def measure(sides):
        """sides: name -> (fn, calls); alternating rounds, median after warm-up."""
        ms = {k: [] for k in sides}
        for r in range(args.warmup + args.rounds):
            for k, (fn, calls) in sides.items():
                v = dev_ms(fn, calls)
                if r >= args.warmup:
                    ms[k].append(v)
        return {k: {"ms_per_call": round(float(np.median(v)), 4), "min_max": [round(min(v), 4), round(max(v), 4)], "calls": sides[k][1]}
                for k, v in ms.items()}

    def forward(nb):
        frames = torch.stack([synth.frame_u8(1080, 1920, seed=s) for s in range(nb)]).to(det.device)
        return frames, eng.forward(list(frames))

    out = {"bench": "nms_batch", "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "warmup": args.warmup,
           "weights": args.weights, "deployed": [], "test": []}
    # ---- the deployed thresholds: the loop against batched=True
    for nb in args.deployed_nb:
        frames, p = forward(nb)
        a = (0.25, 0.35, [0, 1, 2], True)
        eng.nms_enqueue(p, *a)
        want = (p["dets"].clone(), p["count"].clone())
        p["dets"].zero_(); p["count"].fill_(-1)
        eng.nms_enqueue(p, *a, batched=True)
        counts = p["count"].tolist()
        assert torch.equal(p["count"], want[1]), "batched and per-image counts differ"
        assert all(torch.equal(p["dets"][i * 300:i * 300 + k], want[0][i * 300:i * 300 + k]) for i, k in enumerate(counts)), \
            "batched and per-image boxes differ"
        loop = lambda: eng.nms_enqueue(p, *a)                          # noqa: E731
        m = measure({"loop_a": (loop, 20), "batched": (lambda: eng.nms_enqueue(p, *a, batched=True), 20), "loop_b": (loop, 20)})
        la, lb, bt = m["loop_a"]["ms_per_call"], m["loop_b"]["ms_per_call"], m["batched"]["ms_per_call"]
        row = {"nb": nb, "n": p["n_pred"], "kept_per_image_mean": round(float(np.mean(counts)), 2), "same_bytes": True, **m,
               "loop_over_batched": round(min(la, lb) / bt, 3), "loop_a_over_loop_b": round(la / lb, 3)}
        out["deployed"].append(row)
        print(json.dumps(row), file=sys.stderr)
        del frames
    # ---- test.py's protocol: one call against nb calls with nb = 1
    for nb in args.test_nb:
        frames, p = forward(nb)
        n, no, nc = p["n_pred"], eng.no, eng.nc
        a = (0.001, 0.65, None, False)
        eng.nms_enqueue(p, *a, multi_label=True)
        torch.cuda.synchronize()
        cand = p["nms_batch_ws"][1][:nb * 4].view(torch.int32).tolist()
        want = (p["dets"].clone(), p["count"].clone())
        ws1 = torch.empty(lib.hm_nms_batch_workspace_bytes(1, n, nc, 1), dtype=torch.uint8, device=det.device)

        def serial():
            for i in range(nb):
                L.check(lib.hm_yolo_nms_batch(p["pred"].data_ptr() + i * n * no * 4, n * no, 1, n, nc, 0.001, 0.65, 0xFFFFFFFF, 0, 1, 300,
                                              C.byref(p["lp"]), p["dets"].data_ptr() + i * 300 * 24, 300, p["count"].data_ptr() + i * 4,
                                              ws1.data_ptr(), ws1.numel(), L.current_stream()), "hm_yolo_nms_batch")

        p["dets"].zero_(); p["count"].fill_(-1)
        serial()
        counts = p["count"].tolist()
        assert torch.equal(p["count"], want[1]) and all(torch.equal(p["dets"][i * 300:i * 300 + k], want[0][i * 300:i * 300 + k])
                                                        for i, k in enumerate(counts)), "one call and nb calls differ"
        m = measure({"batch": (lambda: eng.nms_enqueue(p, *a, multi_label=True), 2), "serial": (serial, 1),
                     "forward": (lambda: eng.forward(list(frames)), 2)})
        bt = m["batch"]["ms_per_call"]
        row = {"nb": nb, "n": n, "nc": nc, "candidates_per_image": {"min": min(cand), "mean": round(float(np.mean(cand)), 1), "max": max(cand)},
               "images_sorted_in_workspace": sum(c > 16384 for c in cand), "images_cut_to_30000": sum(c > 30000 for c in cand),
               "kept_per_image_mean": round(float(np.mean(counts)), 2), "same_bytes": True, **m,
               "serial_over_batch": round(m["serial"]["ms_per_call"] / bt, 3), "batch_ms_per_frame": round(bt / nb, 4),
               "batch_over_forward": round(bt / m["forward"]["ms_per_call"], 3)}
        out["test"].append(row)
        print(json.dumps(row), file=sys.stderr)
        del frames
    print(json.dumps(out))


if __name__ == "__main__":
    main()
