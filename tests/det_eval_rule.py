"""The CPU rule of the detector evaluation (numpy only): the statement hm_det_match, hm_det_ap and hm_det_ap_curve are held to.

fp32 for the IoU and the matching, fp64 for the AP.  It restates yolo/yolov7/test.py:178-209, utils/metrics.py:18-110 and
general.py:447-469 of the reference the way include/hamer_hip.h does, quirks included:

  * IoU: inter = clamp(min(x2) - max(x1), 0) * clamp(min(y2) - max(y1), 0), iou = inter / (area1 + area2 - inter), fp32, each
    operation rounded on its own; min / max hand a NaN on, as torch's do.
  * the label classes in ascending order, within a class its predictions in stored order; a prediction takes its best-IoU
    target of that class (lowest index on a tie); a NaN in its row makes it unmatched (torch.max hands the NaN on, and
    `NaN > iouv[0]` is false); it is assigned only when iou > iouv[0] strictly and the target is free; no second best; the walk
    of the image stops once every label is taken.
  * ap_per_class: stable sort by descending confidence (the one place narrower than the reference, whose argsort leaves ties
    unspecified); integer cumulative counts; recall = tpc / (n_l + 1e-16); precision = tpc / (tpc + fpc); np.interp semantics
    written out in `interp` below; the reference's sentinels; 101-point trapezoid.

The AP half with exactly these np.interp semantics was compared with the reference's own ap_per_class on 40 random cases
(1..2000 predictions, 1..100 labels, distinct confidences): 0.0 difference in all five returns.  The matching loop is inline in
the reference's test() and cannot be called; it is restated from the text.
"""
import numpy as np

F = np.float32


def _tmin(a, b):
    return a if a != a else b if b != b else (a if a < b else b)


def _tmax(a, b):
    return a if a != a else b if b != b else (a if a > b else b)


def box_iou_pair(b1, b2):
    """general.py:447-469 for one pair of xyxy boxes, fp32 scalars in, fp32 out."""
    with np.errstate(all="ignore"):
        b1 = [F(v) for v in b1]
        b2 = [F(v) for v in b2]
        area1 = F(F(b1[2] - b1[0]) * F(b1[3] - b1[1]))
        area2 = F(F(b2[2] - b2[0]) * F(b2[3] - b2[1]))
        w = F(_tmin(b1[2], b2[2]) - _tmax(b1[0], b2[0]))
        h = F(_tmin(b1[3], b2[3]) - _tmax(b1[1], b2[1]))
        w = F(0) if w < 0 else w
        h = F(0) if h < 0 else h
        inter = F(w * h)
        return F(inter / F(F(area1 + area2) - inter))


def box_iou(box1, box2):
    out = np.zeros((len(box1), len(box2)), F)
    for i, a in enumerate(box1):
        for j, b in enumerate(box2):
            out[i, j] = box_iou_pair(a, b)
    return out


def match_image(pred, labels, iouv):
    """pred (np, 6) xyxy conf cls, labels (nl, 5) cls xyxy, fp32 -> correct (np, niou) u8, best_iou (np,) f32, matched (np,) i32."""
    pred = np.asarray(pred, F).reshape(-1, 6)
    labels = np.asarray(labels, F).reshape(-1, 5)
    iouv = np.asarray(iouv, F)
    n, nl = len(pred), len(labels)
    correct = np.zeros((n, len(iouv)), np.uint8)
    best = np.zeros(n, F)
    matched = np.full(n, -1, np.int32)
    # the row maximum of every prediction that has a label of its class (also of those the walk never reaches)
    arg = np.full(n, -1, np.int64)
    for i in range(n):
        ts = [t for t in range(nl) if labels[t, 0] == pred[i, 5]]
        if not ts:
            continue
        ious = [box_iou_pair(pred[i, :4], labels[t, 1:5]) for t in ts]
        if any(v != v for v in ious):
            best[i] = F(np.nan)
            continue
        k = int(np.argmax(np.asarray(ious, F)))                      # first maximum
        best[i], arg[i] = ious[k], ts[k]
    detected = []
    done = False
    for cls in np.unique(labels[:, 0][~np.isnan(labels[:, 0])]) if nl else []:
        if done:
            break
        taken = set()
        for i in range(n):
            if pred[i, 5] != cls or arg[i] < 0 or not best[i] > iouv[0]:
                continue
            d = int(arg[i])
            if d not in taken:
                taken.add(d)
                detected.append(d)
                matched[i] = d
                correct[i] = best[i] > iouv
                if len(detected) == nl:
                    done = True
                    break
    return correct, best, matched


def match_batch(pred, pred_count, labels, label_count, iouv):
    """The whole of hm_det_match: counts clamped, rows past the count 0 / 0 / -1."""
    pred = np.asarray(pred, F)
    labels = np.asarray(labels, F)
    N, stride = pred.shape[:2]
    lmax = labels.shape[1]
    niou = len(iouv)
    correct = np.zeros((N, stride, niou), np.uint8)
    best = np.zeros((N, stride), F)
    matched = np.full((N, stride), -1, np.int32)
    for i in range(N):
        n = min(max(int(pred_count[i]), 0), stride)
        nl = min(max(int(label_count[i]), 0), lmax)
        c, b, m = match_image(pred[i, :n], labels[i, :nl], iouv)
        correct[i, :n], best[i, :n], matched[i, :n] = c, b, m
    return correct, best, matched


def interp(x, xp, fp, left=None):
    """np.interp's semantics, written out: the right-most knot j with xp[j] <= x gives
    fp[j] + (x - xp[j]) * ((fp[j+1] - fp[j]) / (xp[j+1] - xp[j])); x >= xp[-1] gives fp[-1]; x < xp[0] gives left (fp[0])."""
    xp = np.asarray(xp, np.float64)
    fp = np.asarray(fp, np.float64)
    out = np.empty(len(x), np.float64)
    for k, xv in enumerate(np.asarray(x, np.float64)):
        if xv >= xp[-1]:
            out[k] = fp[-1]
        elif xv < xp[0]:
            out[k] = fp[0] if left is None else left
        else:
            j = int(np.searchsorted(xp, xv, side="right")) - 1
            out[k] = fp[j] + (xv - xp[j]) * ((fp[j + 1] - fp[j]) / (xp[j + 1] - xp[j]))
    return out


def compute_ap(recall, precision, v5_metric=False):
    recall = np.asarray(recall, np.float64)
    precision = np.asarray(precision, np.float64)
    mrec = np.concatenate(([0.0], recall, [1.0 if v5_metric else recall[-1] + 0.01]))
    mpre = np.concatenate(([1.0], precision, [0.0]))
    mpre = np.flip(np.maximum.accumulate(np.flip(mpre)))
    x = np.linspace(0, 1, 101)
    y = interp(x, mrec, mpre)
    ap = float((np.diff(x) * (y[1:] + y[:-1]) / 2.0).sum())
    return ap, mpre, mrec


def ap_curves(tp, conf, pred_cls, target_cls, v5_metric=False):
    """(ap [nc][niou], p [nc][1000], r [nc][1000], unique_classes): metrics.py:33-65 with a stable sort."""
    tp = np.asarray(tp).astype(bool).reshape(len(conf), -1)
    conf = np.asarray(conf)
    pred_cls = np.asarray(pred_cls)
    target_cls = np.asarray(target_cls)
    i = np.argsort(-conf, kind="stable")
    tp, conf, pred_cls = tp[i], conf[i], pred_cls[i]
    unique_classes = np.unique(target_cls)
    nc = len(unique_classes)
    px = np.linspace(0, 1, 1000)
    ap, p, r = np.zeros((nc, tp.shape[1])), np.zeros((nc, 1000)), np.zeros((nc, 1000))
    for ci, c in enumerate(unique_classes):
        sel = pred_cls == c
        n_l = int((target_cls == c).sum())
        if sel.sum() == 0 or n_l == 0:
            continue
        tpc = tp[sel].astype(np.int64).cumsum(0)
        fpc = (1 - tp[sel].astype(np.int64)).cumsum(0)
        recall = tpc / (n_l + 1e-16)
        precision = tpc / (tpc + fpc)
        xp = -conf[sel].astype(np.float64)
        r[ci] = interp(-px, xp, recall[:, 0], left=0.0)
        p[ci] = interp(-px, xp, precision[:, 0], left=1.0)
        for j in range(tp.shape[1]):
            ap[ci, j] = compute_ap(recall[:, j], precision[:, j], v5_metric)[0]
    return ap, p, r, unique_classes


def ap_per_class(tp, conf, pred_cls, target_cls, v5_metric=False):
    ap, p, r, uc = ap_curves(tp, conf, pred_cls, target_cls, v5_metric)
    f1 = 2 * p * r / (p + r + 1e-16)
    i = int(f1.mean(0).argmax()) if len(uc) else 0
    return p[:, i], r[:, i], ap, f1[:, i], uc.astype("int32"), i
