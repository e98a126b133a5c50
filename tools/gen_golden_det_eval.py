#!/usr/bin/env python3
"""Generate tests/golden/det_eval.npz from the REFERENCE's yolo/yolov7/utils/metrics.py and general.py (imported from the
reference tree with the cv2 / torchvision shims of tools/gen_golden_yolo.py; numpy and torch only; CPU).

Per case: the inputs (tp [P][10] u8, conf fp32, pred_cls, target_cls) and the reference's ``ap_per_class`` returns for both
``v5_metric`` values; ``compute_ap`` (both values) on the class-0, threshold-0 curve of some cases; ``box_iou`` for a few box
sets.  Confidences are distinct in every stored case.  A seed is kept only if the largest ``f1.mean(0)`` exceeds every value
not bit-equal to it by at least 1e-9, so that the arg-max cannot hinge on rounding; the seed of a case is the first that
meets this.  Data only, no code."""
import os
import sys
import types

os.environ.setdefault("MPLBACKEND", "Agg")
import numpy as np  # noqa: E402
import torch  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import det_eval_rule as DR  # noqa: E402
from tools.gen_golden_rootnet import REF  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "det_eval.npz")
GAP = 1e-9
NIOU = 10

# name -> (labels per target class {class: n_l}, predictions per class {class: (n_pred, n_tp)}, leading false positives)
CASES = {
    "nl4": ({0: 4}, {0: (12, 4)}, 0),
    "nl10": ({0: 10}, {0: (30, 7)}, 0),
    "three": ({0: 17, 1: 40, 2: 9}, {0: (60, 12), 1: (110, 31), 2: (30, 9)}, 0),
    "class_without_pred": ({0: 6, 1: 5, 2: 8}, {0: (20, 5), 2: (25, 6)}, 0),
    "class_without_label": ({0: 6, 2: 8}, {0: (20, 5), 1: (15, 0), 2: (25, 6)}, 0),
    "single_tp": ({0: 1}, {0: (1, 1)}, 0),
    "single_fp": ({0: 3}, {0: (1, 0)}, 0),
    "large": ({0: 100, 1: 87, 2: 93}, {0: (700, 81), 1: (640, 60), 2: (660, 90)}, 0),
    "all_tp": ({0: 20, 1: 5}, {0: (20, 20), 1: (5, 5)}, 0),
    "one_class_all_fp": ({0: 9, 1: 4}, {0: (40, 8), 1: (11, 0)}, 0),
    "p257": ({1: 50, 2: 64}, {1: (128, 40), 2: (129, 64)}, 0),
    "leading_fp": ({0: 10, 1: 4}, {0: (25, 10), 1: (9, 3)}, 5),
}
CURVES = ("nl4", "nl10", "three", "single_tp", "single_fp", "leading_fp")


def load_reference():
    cv2 = types.ModuleType("cv2"); cv2.setNumThreads = lambda n: None
    sys.modules["cv2"] = cv2
    for name in ("torchvision", "torchvision.ops", "torchvision.utils", "torchvision.models", "torchvision.transforms", "seaborn"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["torchvision"].ops = sys.modules["torchvision.ops"]
    sys.path.insert(0, REF)
    sys.path.insert(0, os.path.join(REF, "yolo"))
    from yolo.yolov7.utils import general, metrics
    return metrics, general


def make_case(spec, seed):
    labels, preds, lead = spec
    rng = np.random.default_rng(seed)
    target_cls = np.concatenate([np.full(n, c, np.float64) for c, n in labels.items()])
    rows = []
    for c, (n, ntp) in preds.items():
        level = np.zeros(n, np.int64)                                  # thresholds passed: correct = a prefix of the ten
        level[rng.choice(n, ntp, replace=False)] = rng.integers(1, NIOU + 1, ntp)
        rows += [(c, lv) for lv in level]
    P = len(rows)
    order = rng.permutation(P)
    pred_cls = np.array([rows[i][0] for i in order], np.float32)
    level = np.array([rows[i][1] for i in order])
    tp = (level[:, None] > np.arange(NIOU)[None, :]).astype(np.uint8)
    conf = rng.uniform(0.02, 0.999, P).astype(np.float32)
    if lead:                                                           # the most confident predictions are false positives
        top = np.argsort(-conf)[:lead]
        tp[top] = 0
    return tp, conf, pred_cls, target_cls


def kept(tp, conf, pred_cls, target_cls):
    if len(np.unique(conf)) != len(conf):
        return False
    for v5 in (False, True):
        _, p, r, _ = DR.ap_curves(tp, conf, pred_cls, target_cls, v5)
        m = (2 * p * r / (p + r + 1e-16)).mean(0)
        rest = m[m != m.max()]
        if len(rest) and m.max() - rest.max() < GAP:
            return False
    return True


def main():
    metrics, general = load_reference()
    out = {"cases": np.array(list(CASES)), "curves": np.array(CURVES)}
    for name, spec in CASES.items():
        seed = 0
        while not kept(*make_case(spec, seed)):
            seed += 1
        tp, conf, pred_cls, target_cls = make_case(spec, seed)
        out[f"{name}/seed"] = np.int64(seed)
        out[f"{name}/tp"], out[f"{name}/conf"], out[f"{name}/pred_cls"], out[f"{name}/target_cls"] = tp, conf, pred_cls, target_cls
        for v5 in (False, True):
            p, r, ap, f1, cls = metrics.ap_per_class(tp.astype(bool), conf, pred_cls, target_cls, v5_metric=v5)
            k = f"{name}/v5_{int(v5)}"
            out[k + "/p"], out[k + "/r"], out[k + "/ap"], out[k + "/f1"], out[k + "/classes"] = p, r, ap, f1, cls
            got = DR.ap_per_class(tp, conf, pred_cls, target_cls, v5)
            dist = max(float(np.abs(np.asarray(a) - np.asarray(b)).max()) for a, b in zip(got[:4], (p, r, ap, f1)))
            print(f"{name:22s} v5={int(v5)} seed {seed} P {len(conf):5d}  rule - reference: {dist:.3g}")
        if name in CURVES:
            st = np.argsort(-conf, kind="stable")
            c0 = np.unique(target_cls)[0]
            sel = pred_cls[st] == c0
            t0 = tp[st][sel][:, 0].astype(np.int64)
            tpc, fpc = t0.cumsum(), (1 - t0).cumsum()
            recall, precision = tpc / ((target_cls == c0).sum() + 1e-16), tpc / (tpc + fpc)
            out[f"{name}/curve/recall"], out[f"{name}/curve/precision"] = recall, precision
            for v5 in (False, True):
                ap, mpre, mrec = metrics.compute_ap(recall, precision, v5_metric=v5)
                k = f"{name}/curve/v5_{int(v5)}"
                out[k + "/ap"], out[k + "/mpre"], out[k + "/mrec"] = np.float64(ap), mpre, mrec
    rng = np.random.default_rng(7)

    def boxes(n, scale):
        xy = rng.uniform(0, scale, (n, 2))
        wh = rng.uniform(0.02 * scale, 0.4 * scale, (n, 2))
        return np.concatenate([xy, xy + wh], 1).astype(np.float32)

    sets = {"pixels": (boxes(9, 640.0), boxes(7, 640.0)), "normalised": (boxes(5, 1.0), boxes(11, 1.0)),
            "special": (np.array([[0, 0, 2, 1], [0, 0, 1, 1], [3, 3, 3, 3], [10, 10, 20, 20]], np.float32),
                        np.array([[0, 0, 1, 1], [1, 0, 2, 1], [3, 3, 3, 3], [12, 12, 18, 18], [30, 30, 40, 40]], np.float32))}
    out["iou_sets"] = np.array(list(sets))
    for name, (a, b) in sets.items():
        out[f"iou/{name}/a"], out[f"iou/{name}/b"] = a, b
        out[f"iou/{name}/iou"] = general.box_iou(torch.from_numpy(a), torch.from_numpy(b)).numpy()
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
