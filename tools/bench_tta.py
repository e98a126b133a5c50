"""The detector pass with and without test-time augmentation, on passes of seeded 1080p frames
through the synthetic detector (letterboxed to 384 x 640; the TTA pass adds 320 x 544 mirrored and 288 x 448).

  python tools/bench_tta.py [--nb 16 48] [--rounds 10] [--warmup 3] [--precise] [--weights synthetic:2:-2.2:0]

Per ``--nb`` (frames per pass), all in one process, the variants alternating inside each round:
  plain      YoloEngine.forward(frames): letterbox, the graph, three decode launches
  tta        YoloEngine.forward(frames, tta=True): letterbox, two hm_tta_scale, three graphs, nine decode launches
  scale_<s>  one scale's graph and its three decode launches alone (the three scales' shares of the TTA pass)
  resize_<s> one hm_tta_scale launch alone, with the bytes it has to move (the full-size image read once, the scaled image
             written once, 8 channels per pixel as stored) over its time -- at these sizes both images fit the 256 MiB
             Infinity Cache, so the figure is no HBM rate
  nms_plain, nms_tta  YoloEngine.nms_enqueue at the deployed thresholds on the plain (15120 rows) and the TTA pred (33768)
The input-area ratio of the three scales is (245760 + 174080 + 129024) / 245760 = 2.233; the tool prints the measured
tta / plain beside it.  Every figure is the median over ``--rounds`` of the time between two device events around ``calls``
back-to-back enqueues, after ``--warmup`` rounds.  One JSON line per pass size on stderr, one at the end."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

AREA_RATIO = (245760 + 174080 + 129024) / 245760


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nb", type=int, nargs="+", default=[16, 48])
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--precise", action="store_true", help="the fp32 route")
    ap.add_argument("--weights", type=str, default="synthetic:2:-2.2:0")
    args = ap.parse_args()
    import ctypes as C
    import torch
    from hamer_yolo_amd import lib as L
    from hamer_yolo_amd import synth
    from hamer_yolo_amd.yolo import arch
    from hamer_yolo_amd.yolo.detector import Detector
    if not torch.cuda.is_available():
        raise SystemExit("bench_tta.py measures on the GPU; none is visible")

    class Cfg:
        weights = args.weights; imgsz = 640; augment = True; conf_thres = 0.25; iou_thres = 0.35
        classes = [0, 1, 2]; agnostic_nms = True; device = "cuda"; save_path = "./output"

    det = Detector(Cfg, precise=args.precise)
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

    out = {"bench": "tta", "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "warmup": args.warmup,
           "weights": args.weights, "route": "fp32" if args.precise else "fp16", "input_area_ratio": round(AREA_RATIO, 3), "passes": []}
    for nb in args.nb:
        frames = list(torch.stack([synth.frame_u8(1080, 1920, seed=s) for s in range(nb)]).to(det.device))
        plain = eng.forward(frames)
        ref = plain["pred"].clone()
        p = eng.forward(frames, tta=True)
        n1, n = plain["n_pred"], p["n_pred"]
        assert torch.equal(p["pred"].reshape(nb, n, eng.no)[:, :n1].reshape(-1, eng.no), ref), "the TTA pass does not hold the plain pass"
        lp, st = p["lp"], L.current_stream()

        def graph(t):
            def run():
                L.check(lib.hm_yolo_run(t["ops"], t["n_ops"], st), "hm_yolo_run")
                row0 = t["row0"]
                for l, (raw, hh, ww) in enumerate(t["raws"]):
                    anc = (C.c_float * 6)(*eng.anchors[l])
                    L.check(lib.hm_yolo_decode_batch_tta(raw.data_ptr(), 3 * eng.no, p["pred"].data_ptr(), row0, hh, ww, eng.nc,
                                                         float(arch.STRIDES[l]), anc, nb, n, t["ratio"], int(t["flip"]), float(lp.out_w),
                                                         st), "hm_yolo_decode_batch_tta")
                    row0 += 3 * hh * ww
            return run

        def resize(t):
            return lambda: L.check(lib.hm_tta_scale(p["img_ptr"], t["img_ptr"], t["tab"].data_ptr(), nb, lp.out_h, lp.out_w, t["ratio"],
                                                    eng.stride, eng.dt, st), "hm_tta_scale")

        nms = (0.25, 0.35, [0, 1, 2], True)
        sides = {"plain": (lambda: eng.forward(frames), 4), "tta": (lambda: eng.forward(frames, tta=True), 4)}
        for t in p["tta"]:
            sides[f"scale_{t['ratio']:g}"] = (graph(t), 4)
        for t in p["tta"][1:]:
            sides[f"resize_{t['ratio']:g}"] = (resize(t), 50)
        sides["nms_plain"] = (lambda: eng.nms_enqueue(plain, *nms), 4)
        sides["nms_tta"] = (lambda: eng.nms_enqueue(p, *nms), 4)
        m = measure(sides)
        eng.forward(frames, tta=True)
        eng.nms_enqueue(p, *nms)
        kept_tta = float(np.mean(p["count"].tolist()))
        eng.forward(frames)
        eng.nms_enqueue(plain, *nms)
        kept_plain = float(np.mean(plain["count"].tolist()))
        tp, tt = m["plain"]["ms_per_call"], m["tta"]["ms_per_call"]
        g = [m[f"scale_{t['ratio']:g}"]["ms_per_call"] for t in p["tta"]]
        row = {"nb": nb, "rows_plain": n1, "rows_tta": n, **m, "tta_over_plain": round(tt / tp, 3), "input_area_ratio": round(AREA_RATIO, 3),
               "plain_ms_per_frame": round(tp / nb, 4), "tta_ms_per_frame": round(tt / nb, 4),
               "scale_share_of_tta": {f"{t['ratio']:g}": round(v / tt, 3) for t, v in zip(p["tta"], g)},
               "scale_over_full_size_graph": {f"{t['ratio']:g}": round(v / g[0], 3) for t, v in zip(p["tta"], g)},
               "scale_area_over_full_size": {f"{t['ratio']:g}": round(t["h"] * t["w"] / (lp.out_h * lp.out_w), 3) for t in p["tta"]},
               "kept_per_image_mean": {"plain": round(kept_plain, 2), "tta": round(kept_tta, 2)}, "resize": {}}
        for t in p["tta"][1:]:
            byts = nb * 8 * eng.esz * (lp.out_h * lp.out_w + t["h"] * t["w"])
            ms = m[f"resize_{t['ratio']:g}"]["ms_per_call"]
            row["resize"][f"{t['ratio']:g}"] = {"to": [t["h"], t["w"]], "bytes": byts, "ms": ms, "gb_per_s": round(byts / ms / 1e6, 1)}
        out["passes"].append(row)
        print(json.dumps(row), file=sys.stderr)
        del frames
    print(json.dumps(out))


if __name__ == "__main__":
    main()
