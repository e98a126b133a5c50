"""Score a detector on a labelled folder: P, R, mAP@.5 and mAP@.5:.95 as yolo/yolov7/test.py prints them.

    python -m hamer_yolo_amd.evaluate_det --pred DIR --labels DIR [--size W H] [--json out.json]
    python -m hamer_yolo_amd.evaluate_det --images DIR --labels DIR [--weights W] [--precise-detector]
                                          [--protocol {deployed,test}] [--multi-label] [--augment]
                                          [--conf-thres C] [--iou-thres I] [--save-txt DIR [--save-conf]]
                                          [--det-frames N] [--json out.json]

Label and prediction files are the reference's text format (test.py:146-152): one ``<stem>.txt`` per image, a line being
``cls cx cy w h [conf]`` in normalised xywh; prediction files need the ``conf`` column (``--save-conf``).

``--pred``: the images are the prediction files (``--save-txt`` here writes one per image, empty when nothing was detected).
Without ``--size`` the boxes stay normalised, where IoU equals the pixel IoU up to rounding; ``--size W H`` scales both sides
to pixels first.  ``--images``: the detector runs over the folder in batched passes of equally sized frames and every pass is
scored on the device from the plan's ``dets`` / ``count`` (hm_det_match), with no host round trip per image.

An image without a label file has zero labels.  A label file without an image is reported and skipped.

``--protocol deployed`` (the default) scores at the deployed thresholds (config/yolo_config.py: conf 0.25, IoU 0.35, best class
only, NMS as configured there).  A PR curve cut at conf 0.25 ends early, so that mAP is lower than the one test.py prints for
the same weights.  ``--protocol test`` is test.py's own (test.py:125): conf 0.001, IoU 0.65, multi-label candidates, class-aware
NMS over all classes, 300 boxes per image, then the same matching and AP; the whole pass goes through one hm_yolo_nms_batch
call.  An explicit ``--conf-thres`` / ``--iou-thres`` still wins, and ``--multi-label`` alone adds the multi-label branch to the
deployed thresholds.  ``--augment`` (test.py's name, either protocol) runs the detector with test-time augmentation
(``Detector(tta=True)``: scales 1, 0.83 mirrored, 0.67 and one NMS, yolo.py:589-605).  Not reproduced from test.py: its
dataloader's letterbox (``rect``, pad 0.5) -- the detector's own letterbox is used -- ``--single-cls``, ``--save-hybrid`` and
the COCO JSON, and ``--augment`` unless it is given.  The table says which protocol and thresholds it was made with.
"""
from __future__ import annotations

import argparse
import glob
import json
import os
from typing import Dict, List, Optional

import numpy as np

BATCH = 64                # images per hm_det_match launch in --pred mode
DET_FRAMES = 16           # frames per detector pass in --images mode
HEADER = ('%20s' + '%12s' * 6) % ('Class', 'Images', 'Labels', 'P', 'R', 'mAP@.5', 'mAP@.5:.95')      # test.py:100
PF = '%20s' + '%12i' * 2 + '%12.3g' * 4                                                               # test.py:232


def _stems(folder: str) -> Dict[str, str]:
    return {os.path.splitext(os.path.basename(p))[0]: p for p in sorted(glob.glob(os.path.join(folder, "*.txt")))}


def _pack(rows: List[np.ndarray], width: int, depth: int):
    """list of (n_i, width) arrays -> ((N, depth, width) fp32, (N,) int32)."""
    out = np.zeros((len(rows), depth, width), np.float32)
    for i, r in enumerate(rows):
        out[i, :len(r)] = r
    return out, np.array([len(r) for r in rows], np.int32)


def _result_dict(res: Dict, names: List[str], extra: Dict) -> Dict:
    per_class = [{"class": int(c), "name": names[int(c)] if int(c) < len(names) else str(int(c)), "labels": int(res["nt"][int(c)]),
                  "p": float(res["p"][i]), "r": float(res["r"][i]), "ap50": float(res["ap50"][i]), "ap": float(res["ap"][i])}
                 for i, c in enumerate(res["ap_class"])]
    out = {"seen": int(res["seen"]), "labels": int(res["nt"].sum()), "nt": [int(v) for v in res["nt"]], "mp": res["mp"],
           "mr": res["mr"], "map50": res["map50"], "map": res["map"], "classes": per_class}
    out.update(extra)
    return out


def format_table(result: Dict) -> str:
    """test.py:100, :232-238: the header, the ``all`` line, one line per class."""
    lines = [HEADER, PF % ('all', result["seen"], result["labels"], result["mp"], result["mr"], result["map50"], result["map"])]
    for c in result["classes"]:
        lines.append(PF % (c["name"], result["seen"], c["labels"], c["p"], c["r"], c["ap50"], c["ap"]))
    return "\n".join(lines)


def score_folders(pred_dir: str, label_dir: str, size=None, json_path: Optional[str] = None, nc: Optional[int] = None) -> Dict:
    """Score the prediction files of ``pred_dir`` against the label files of ``label_dir``.  Returns ``{'seen', 'labels',
    'nt', 'mp', 'mr', 'map50', 'map', 'classes': [{'class', 'name', 'labels', 'p', 'r', 'ap50', 'ap'}], 'only_labels':
    [stems skipped], 'size'}``.  ``size=(W, H)``: both sides scaled to pixels (fp32); None: normalised coordinates."""
    from .yolo import metrics as M
    preds, labels = _stems(pred_dir), _stems(label_dir)
    stems = sorted(preds)
    only_labels = [s for s in sorted(labels) if s not in preds]
    P = [M.load_label_file(preds[s], conf=True) for s in stems]
    T = [M.load_label_file(labels[s]) if s in labels else np.zeros((0, 5), np.float32) for s in stems]
    if size is not None:
        g = np.array([size[0], size[1], size[0], size[1]], np.float32)
        for p in P:
            p[:, :4] *= g
        for t in T:
            t[:, 1:5] *= g
    stride, lmax = max([len(p) for p in P] + [1]), max([len(t) for t in T] + [1])
    if stride > M.MAX_PRED_ROWS or lmax > M.MAX_LABEL_ROWS:
        raise ValueError(f"an image has {stride} predictions / {lmax} labels: the limits are {M.MAX_PRED_ROWS} / {M.MAX_LABEL_ROWS}")
    top = max([int(p[:, 5].max()) for p in P if len(p)] + [int(t[:, 0].max()) for t in T if len(t)] + [0])
    nc = top + 1 if nc is None else int(nc)
    ev = M.DetEvaluator(nc)
    for i in range(0, len(stems), BATCH):
        pr, pc = _pack(P[i:i + BATCH], 6, stride)
        lb, lc = _pack(T[i:i + BATCH], 5, lmax)
        ev(pr, pc, lb, lc)
    result = _result_dict(ev.result(), [str(i) for i in range(nc)],
                          {"only_labels": only_labels, "size": None if size is None else [int(size[0]), int(size[1])]})
    if json_path:
        with open(json_path, "w") as f:
            json.dump(result, f, indent=1)
    return result


def score_images(image_dir: str, label_dir: str, detector, save_txt: Optional[str] = None, save_conf: bool = False,
                 json_path: Optional[str] = None, det_frames: int = DET_FRAMES, multi_label: bool = False,
                 agnostic: Optional[bool] = None, protocol: str = "deployed") -> Dict:
    """Run ``detector`` over the images of ``image_dir`` in batched passes (runs of consecutive equally sized frames, up to
    ``det_frames``) and score every pass on the device against the label files of ``label_dir``.  ``save_txt``: also write the
    predictions, one file per image, in the label format (this copies each pass's boxes to the host).  ``multi_label``: the
    reference's multi-label NMS branch (the pass then goes through one hm_yolo_nms_batch call); ``agnostic``: None reads
    ``detector.opt.agnostic_nms``; ``protocol`` is recorded in the result, and so is the detector's ``tta`` as ``augment``."""
    import torch
    from .infer import _imread_bgr, _list_images
    from .yolo import metrics as M
    paths = _list_images(image_dir)
    labels = _stems(label_dir)
    stems = [os.path.splitext(os.path.basename(p))[0] for p in paths]
    only_labels = [s for s in sorted(labels) if s not in set(stems)]
    opt, eng = detector.opt, detector.engine
    ev = M.DetEvaluator(eng.nc)
    agnostic = bool(opt.agnostic_nms) if agnostic is None else bool(agnostic)
    if save_txt:
        os.makedirs(save_txt, exist_ok=True)
    unreadable = []
    i = 0
    pending = None                                                     # one decoded frame carried over a size change
    while i < len(paths) or pending is not None:
        run = []
        while len(run) < det_frames and (pending is not None or i < len(paths)):
            if pending is None:
                im = _imread_bgr(paths[i])
                item = (stems[i], im)
                i += 1
                if im is None:
                    unreadable.append(item[0])
                    continue
            else:
                item, pending = pending, None
            if run and item[1].shape != run[0][1].shape:
                pending = item
                break
            run.append(item)
        if not run:
            continue
        H, W = run[0][1].shape[:2]
        frames = torch.from_numpy(np.stack([im for _, im in run])).to(detector.device)
        p = eng.forward(list(frames), tta=bool(getattr(detector, "tta", False)))
        eng.nms_enqueue(p, opt.conf_thres, opt.iou_thres, opt.classes, agnostic, scale=True, multi_label=bool(multi_label))
        g = np.array([W, H, W, H], np.float32)
        T = [M.load_label_file(labels[s]) if s in labels else np.zeros((0, 5), np.float32) for s, _ in run]
        for t in T:
            t[:, 1:5] *= g                                             # to the predictions' units: frame pixels
        lmax = max([len(t) for t in T] + [1])
        if lmax > M.MAX_LABEL_ROWS:
            raise ValueError(f"an image has {lmax} labels: the limit is {M.MAX_LABEL_ROWS}")
        lb, lc = _pack(T, 5, lmax)
        ev(p["dets"], p["count"], lb, lc)
        if save_txt:
            counts = p["count"].tolist()
            host = p["dets"].reshape(p["nb"], 300, 6).cpu()
            for k, (s, _) in enumerate(run):
                M.save_label_file(os.path.join(save_txt, s + ".txt"), host[k, :int(counts[k])], size=(W, H), conf=save_conf)
    result = _result_dict(ev.result(), list(eng.names),
                          {"only_labels": only_labels, "unreadable": unreadable, "conf_thres": float(opt.conf_thres),
                           "iou_thres": float(opt.iou_thres), "precise": bool(detector.precise), "protocol": str(protocol),
                           "multi_label": bool(multi_label), "agnostic": agnostic, "augment": bool(getattr(detector, "tta", False))})
    if json_path:
        with open(json_path, "w") as f:
            json.dump(result, f, indent=1)
    return result


def _parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description="score a detector on a labelled folder: P, R, mAP@.5, mAP@.5:.95")
    ap.add_argument('--labels', type=str, required=True, help="folder of label files (<stem>.txt: cls cx cy w h, normalised)")
    ap.add_argument('--pred', type=str, default=None, help="folder of saved prediction files (cls cx cy w h conf) to score")
    ap.add_argument('--images', type=str, default=None, help="folder of images to run the detector over")
    ap.add_argument('--size', type=int, nargs=2, metavar=('W', 'H'), default=None, help="--pred: scale both sides to pixels of this frame size")
    ap.add_argument('--weights', type=str, default=None, help="--images: checkpoint or synthetic:<seed> (default: config/yolo_config.py)")
    ap.add_argument('--precise-detector', action='store_true', help="--images: the fp32 detector route")
    ap.add_argument('--protocol', choices=('deployed', 'test'), default='deployed',
                    help="--images: deployed = the thresholds and NMS of config/yolo_config.py; test = test.py's: conf 0.001, IoU 0.65, "
                         "multi-label, class-aware, all classes")
    ap.add_argument('--multi-label', action='store_true', help="--images: one candidate per (box, class) above the threshold (implied by --protocol test)")
    ap.add_argument('--augment', action='store_true',
                    help="--images: test-time augmentation in the detector (scales 1, 0.83 mirrored, 0.67; one NMS), about 2.2x the detector time")
    ap.add_argument('--conf-thres', type=float, default=None, help="--images: default the protocol's (deployed: yolo_opt.conf_thres; test: 0.001)")
    ap.add_argument('--iou-thres', type=float, default=None, help="--images: NMS IoU, default the protocol's (deployed: yolo_opt.iou_thres; test: 0.65)")
    ap.add_argument('--save-txt', type=str, default=None, help="--images: also write the predictions to this folder in the label format")
    ap.add_argument('--save-conf', action='store_true', help="with --save-txt: append the confidence column (needed to score the files later)")
    ap.add_argument('--det-frames', type=int, default=DET_FRAMES, help="--images: frames per detector pass")
    ap.add_argument('--json', type=str, default=None, help="also write the result to this file")
    return ap


def main(argv=None):
    args = _parser().parse_args(argv)
    if (args.pred is None) == (args.images is None):
        raise SystemExit("give exactly one of --pred DIR and --images DIR")
    if args.pred is not None:
        result = score_folders(args.pred, args.labels, args.size, args.json)
        note = "scored saved predictions: the thresholds are those they were saved with"
    else:
        from .config.yolo_config import yolo_opt
        from .yolo.detector import Detector
        if args.weights:
            yolo_opt.weights = args.weights
        test = args.protocol == 'test'
        if test:                                                       # test.py:125 and its argument defaults
            yolo_opt.conf_thres, yolo_opt.iou_thres, yolo_opt.classes = 0.001, 0.65, None
        if args.conf_thres is not None:
            yolo_opt.conf_thres = args.conf_thres
        if args.iou_thres is not None:
            yolo_opt.iou_thres = args.iou_thres
        result = score_images(args.images, args.labels, Detector(yolo_opt, precise=True if args.precise_detector else None,
                                                                        tta=True if args.augment else None),
                              args.save_txt, args.save_conf, args.json, args.det_frames, multi_label=test or args.multi_label,
                              agnostic=False if test else None, protocol=args.protocol)
        if test:
            note = (f"protocol test: conf_thres {result['conf_thres']:g}, iou_thres {result['iou_thres']:g}, multi-label, class-aware NMS "
                    "over all classes, 300 boxes per image, test.py's matching and AP.  Not reproduced: test.py's dataloader "
                    "letterbox (rect, pad 0.5; the detector's own letterbox is used), "
                    + ("" if result["augment"] else "--augment, ") + "--single-cls, --save-hybrid, COCO JSON")
            if result["augment"]:
                note += ".  --augment: scales 1, 0.83 (mirrored), 0.67 into one NMS"
        else:
            note = (f"conf_thres {result['conf_thres']:g}, iou_thres {result['iou_thres']:g} (the deployed defaults are 0.25 / 0.35; "
                    "test.py's are 0.001 / 0.65 -- a PR curve cut at a higher confidence gives a lower mAP)")
            if args.multi_label:
                note += "; multi-label candidates"
            if result["augment"]:
                note += "; --augment: scales 1, 0.83 (mirrored), 0.67 into one NMS"
    print(format_table(result))
    print(note)
    for s in result["only_labels"]:
        print(f"label file without an image, skipped: {s}")
    return result


if __name__ == '__main__':
    main()
