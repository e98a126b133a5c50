"""non_max_suppression (yolo/yolov7/utils/general.py:611-703, labels=(), merge=False) restated in numpy, fp32 operation by
fp32 operation, both branches -- the rule hm_yolo_nms_batch implements -- and the seeded inputs the NMS tests share.

Per image: rows with obj > conf; scores cls_c * obj (obj itself when nc == 1, which also turns multi_label off); best class
(first maximum) or, multi-label, every class above conf in (row, class) order; class mask; xywh -> xyxy; stable descending
sort by score (equal scores: lower row * nc + class first); the best 30000; greedy suppression on box + cls * 4096 (0 when
agnostic) with IoU = inter / (area_i + area_j - inter), suppressed when IoU > iou (a NaN does not suppress); the first
max_det kept; optionally the letterbox plan's (b - pad) / gain, clamp, round-half-even.
"""
import numpy as np

F = np.float32
MAX_NMS = 30000
MAX_WH = 4096


def nms_image(pred, conf_thres, iou_thres, classes=None, agnostic=False, multi_label=False, max_det=300, plan=None):
    """pred (n, 5+nc) fp32 -> (k, 6) fp32 [x1, y1, x2, y2, conf, cls].  ``plan``: None or (pad_x, pad_y, gain, src_w, src_h)."""
    pred = np.ascontiguousarray(pred, F)
    nc = pred.shape[1] - 5
    multi = bool(multi_label) and nc > 1
    ct, it = F(conf_thres), F(iou_thres)
    rows = np.flatnonzero(pred[:, 4] > ct)
    x = pred[rows]
    sc = x[:, 4:5].copy() if nc == 1 else x[:, 5:] * x[:, 4:5]
    hw, hh = x[:, 2] / F(2), x[:, 3] / F(2)
    box = np.stack([x[:, 0] - hw, x[:, 1] - hh, x[:, 0] + hw, x[:, 1] + hh], 1)
    if multi:
        i, j = np.nonzero(sc > ct)                                     # row-major: (row, class) order
    else:
        i = np.arange(len(rows))
        j = sc.argmax(1) if len(rows) else np.zeros(0, np.int64)        # first maximum
        keep = sc[i, j] > ct
        i, j = i[keep], j[keep]
    if classes is not None:
        keep = np.isin(j, np.asarray(classes, np.int64))
        i, j = i[keep], j[keep]
    conf, b, cls = sc[i, j], box[i], j.astype(F)
    order = np.argsort(-conf, kind="stable")[:MAX_NMS]                  # candidates are in row * nc + class order already
    conf, b, cls = conf[order], b[order], cls[order]
    o = b + (cls * F(0 if agnostic else MAX_WH))[:, None]
    area = (o[:, 2] - o[:, 0]) * (o[:, 3] - o[:, 1])
    dead = np.zeros(len(o), bool)
    kept = []
    for k in range(len(o)):
        if len(kept) >= max_det:
            break
        if dead[k]:
            continue
        kept.append(k)
        w = np.maximum(F(0), np.minimum(o[k, 2], o[k + 1:, 2]) - np.maximum(o[k, 0], o[k + 1:, 0]))
        h = np.maximum(F(0), np.minimum(o[k, 3], o[k + 1:, 3]) - np.maximum(o[k, 1], o[k + 1:, 1]))
        inter = w * h
        with np.errstate(invalid="ignore", divide="ignore"):
            dead[k + 1:] |= inter / ((area[k] + area[k + 1:]) - inter) > it
    kept = np.asarray(kept, np.int64)
    out = np.concatenate([b[kept], conf[kept, None], cls[kept, None]], 1).astype(F).reshape(-1, 6)
    return out if plan is None else scale(out, plan)


def scale(dets, plan):
    """scale_coords + clip + round of the detector (general.py:323-344, detector.py:142) on (k, 6) rows, in fp32."""
    px, py, gain, sw, sh = plan
    pad = np.array([px, py, px, py], F)
    lim = np.array([sw, sh, sw, sh], F)
    out = dets.copy()
    out[:, :4] = np.rint(np.minimum(np.maximum((dets[:, :4] - pad) / F(gain), F(0)), lim))
    return out


def nms(pred, conf_thres, iou_thres, classes=None, agnostic=False, multi_label=False, max_det=300, plan=None):
    """(nb, n, 5+nc) -> list of (k, 6)."""
    return [nms_image(p, conf_thres, iou_thres, classes, agnostic, multi_label, max_det, plan) for p in pred]


def class_mask(classes):
    return 0xFFFFFFFF if classes is None else sum(1 << int(c) for c in classes)


# ------------------------------------------------------------------ seeded inputs
def make_image(rng, n, nc, obj=(0.0, 1.0), cls=(0.0, 1.0), size=(20.0, 120.0), extent=(640.0, 384.0), clusters=0, low_cls=0.0,
               ties=0, distinct=False):
    """One (n, 5+nc) fp32 prediction.  ``clusters``: the centres are that many points with a 2-pixel jitter and the sizes
    100 +- 3 (heavy overlap).  ``low_cls``: this share of the class scores is 1e-5 (below any threshold used here).  ``ties``:
    that many rows get the objectness and class scores of the row before them (another box).  ``distinct``: class scores are
    nudged down one ulp at a time until all n * nc products differ."""
    p = np.zeros((n, 5 + nc), F)
    if clusters:
        c = rng.uniform([100, 100], [extent[0] - 100, extent[1] - 100], (clusters, 2))
        p[:, :2] = c[rng.integers(0, clusters, n)] + rng.uniform(-2, 2, (n, 2))
        p[:, 2:4] = rng.uniform(97, 103, (n, 2))
    else:
        p[:, :2] = rng.uniform([0, 0], extent, (n, 2))
        p[:, 2:4] = rng.uniform(size[0], size[1], (n, 2))
    p[:, 4] = rng.uniform(obj[0], obj[1], n)
    p[:, 5:] = rng.uniform(cls[0], cls[1], (n, nc))
    if low_cls:
        p[:, 5:][rng.uniform(size=(n, nc)) < low_cls] = 1e-5
    if ties:
        r = rng.choice(np.arange(1, n), ties, replace=False)
        p[r, 4:] = p[r - 1, 4:]
    while distinct:
        s = (p[:, 5:] * p[:, 4:5]).ravel()
        _, first, counts = np.unique(s, return_index=True, return_counts=True)
        if (counts == 1).all():
            break
        dup = np.setdiff1d(np.arange(s.size), first)
        v = p[:, 5:].ravel()
        v[dup] = np.nextafter(v[dup], F(0))
        p[:, 5:] = v.reshape(n, nc)
    return p


def pass_nc3(seed, nb, n, ties=8):
    """nb images of n rows, 3 classes: image 1 has no row above 0.001, image 2 (when there) every row above 0.25 in every
    class, the others a mix; ``ties`` duplicated score rows in each."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(nb):
        if i == 1:
            out.append(make_image(rng, n, 3, obj=(0.0, 0.0009)))
        elif i == 2:
            out.append(make_image(rng, n, 3, obj=(0.8, 1.0), cls=(0.5, 1.0), ties=ties))
        else:
            out.append(make_image(rng, n, 3, ties=ties))
    return np.stack(out)


def image_truncated(seed=32, n=1000, nc=32):
    """n * nc = 32000 candidates at conf 0.001, all scores distinct, small boxes spread over 640 x 640: the sort leaves LDS,
    the 30000 cut applies, far more than 300 survive."""
    return make_image(np.random.default_rng(seed), n, nc, obj=(0.5, 1.0), cls=(0.05, 1.0), size=(8.0, 20.0), extent=(640.0, 640.0),
                      distinct=True)


def image_crowded(seed=33, n=1000, nc=32):
    """About 17000 candidates at conf 0.001 in four tight clusters: fewer than 300 survive, the loop walks every candidate."""
    return make_image(np.random.default_rng(seed), n, nc, obj=(0.5, 1.0), cls=(0.05, 1.0), extent=(640.0, 640.0), clusters=4,
                      low_cls=0.47)
