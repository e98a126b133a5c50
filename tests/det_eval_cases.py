"""Inputs shared by tests/test_det_eval_host.py and tests/test_gpu_det_eval.py: the hand-worked matching cases (each with the
answer worked out by hand, stated here and nowhere computed) and seeded generators for the batched cases."""
import numpy as np
import torch

F = np.float32
IOUV = torch.linspace(0.5, 0.95, 10).numpy().copy()                                 # test.py:78, torch's bits


def P(box, cls, conf=0.9):
    return [*box, conf, cls]


def T(box, cls):
    return [cls, *box]


# name -> (pred rows, label rows, matched per prediction, thresholds passed per prediction, best_iou per prediction or None
#          where the value is not a short decimal; NaN where the row holds a NaN)
HAND = {
    # the second prediction's best target (0, IoU 9.5/10.5) is taken; its second best (1, IoU 8.5/11.5 = 0.74) would pass
    "best_target_taken": ([P([0, 0, 10, 10], 0), P([0.5, 0, 10.5, 10], 0)], [T([0, 0, 10, 10], 0), T([2, 0, 12, 10], 0)],
                          [0, -1], [10, 0], [1.0, None]),
    # two identical targets: the lower index is the arg-max; the second prediction finds it taken
    "identical_targets": ([P([0, 0, 10, 10], 1), P([0, 0, 10, 10], 1, 0.8)], [T([0, 0, 10, 10], 1), T([0, 0, 10, 10], 1)],
                          [0, -1], [10, 0], [1.0, 1.0]),
    # inter 1, union 2 + 1 - 1 = 2: IoU exactly 0.5, and `>` is strict
    "iou_exactly_half": ([P([0, 0, 2, 1], 0)], [T([0, 0, 1, 1], 0)], [-1], [0], [0.5]),
    # IoU 77 / 100: above 0.5 .. 0.75, below 0.8
    "prefix_of_six": ([P([0, 0, 10, 10], 2)], [T([0, 0, 10, 7.7], 2)], [0], [6], [None]),
    "class_mismatch": ([P([0, 0, 10, 10], 1)], [T([0, 0, 10, 10], 0)], [-1], [0], [0.0]),
    # classes ascending 0, 1, 2: the class-2 label is the last one taken (by prediction 0) and the walk stops; prediction 3
    # could not have had it anyway
    "three_classes": ([P([40, 0, 50, 10], 2), P([0, 0, 10, 10], 0), P([20, 0, 30, 10], 1), P([40, 0, 50, 10], 2, 0.5)],
                      [T([0, 0, 10, 10], 0), T([20, 0, 30, 10], 1), T([40, 0, 50, 10], 2)], [2, 0, 1, -1], [10, 10, 10, 0],
                      [1.0, 1.0, 1.0, 1.0]),
    # a zero-area prediction against a zero-area label: 0 / 0.  That prediction is unmatched; the other is untouched (its
    # own IoU with the zero-area label is 0 / 100 = 0)
    "nan_pair": ([P([0, 0, 10, 10], 0), P([3, 3, 3, 3], 0)], [T([3, 3, 3, 3], 0), T([0, 0, 10, 10], 0)], [1, -1], [10, 0],
                 [1.0, float("nan")]),
    "one_by_one": ([P([5, 5, 15, 25], 1)], [T([5, 5, 15, 25], 1)], [0], [10], [1.0]),
    "labels_no_predictions": ([], [T([0, 0, 10, 10], 0), T([5, 5, 8, 8], 1)], [], [], []),
    "predictions_no_labels": ([P([0, 0, 10, 10], 0), P([1, 1, 4, 4], 2)], [], [-1, -1], [0, 0], [0.0, 0.0]),
    "neither": ([], [], [], [], []),
}


def hand_arrays(name):
    pred, lab, matched, npass, best = HAND[name]
    return (np.asarray(pred, F).reshape(-1, 6), np.asarray(lab, F).reshape(-1, 5), np.asarray(matched, np.int32),
            np.asarray(npass, np.int64), best)


def check_hand(name, correct, best_iou, matched):
    """correct (n, 10), best_iou (n,), matched (n,) of the case's image against the hand-worked answer."""
    _, _, m, npass, best = hand_arrays(name)
    assert np.array_equal(np.asarray(matched), m), (name, matched)
    want = np.arange(10)[None, :] < npass[:, None]
    assert np.array_equal(np.asarray(correct).astype(bool).reshape(len(m), 10), want), (name, correct)
    for got, b in zip(np.asarray(best_iou), best):
        if b is None:
            continue
        assert (np.isnan(got) and np.isnan(b)) or got == F(b), (name, got, b)


def random_image(rng, n_pred, n_lab, n_cls=3, scale=640.0):
    """n_lab labels and n_pred predictions, most of them jittered copies of a label (so the IoUs spread over 0.3 .. 1 and
    several predictions compete for one label), some with another class, some elsewhere."""
    xy = rng.uniform(0, scale * 0.8, (max(n_lab, 1), 2))
    wh = rng.uniform(scale * 0.03, scale * 0.2, (max(n_lab, 1), 2))
    lab_box = np.concatenate([xy, xy + wh], 1)
    lab_cls = rng.integers(0, n_cls, max(n_lab, 1))
    src = rng.integers(0, max(n_lab, 1), n_pred)
    w = (lab_box[src, 2:] - lab_box[src, :2])
    box = lab_box[src] + rng.normal(size=(n_pred, 4)) * np.concatenate([w, w], 1) * rng.choice([0.01, 0.05, 0.15], (n_pred, 1))
    cls = np.where(rng.uniform(size=n_pred) < 0.85, lab_cls[src], rng.integers(0, n_cls, n_pred))
    conf = rng.uniform(0.05, 1.0, n_pred)
    pred = np.concatenate([box, conf[:, None], cls[:, None]], 1).astype(F)
    labels = np.concatenate([lab_cls[:, None], lab_box], 1).astype(F)[:n_lab]
    return pred, labels


def pack(images, stride, lmax, fill=0.0):
    """[(pred, labels)] -> pred (N, stride, 6), pred_count, labels (N, lmax, 5), label_count; the padding rows hold `fill`."""
    N = len(images)
    pred = np.full((N, stride, 6), fill, F)
    labels = np.full((N, lmax, 5), fill, F)
    pc, lc = np.zeros(N, np.int32), np.zeros(N, np.int32)
    for i, (p, t) in enumerate(images):
        pred[i, :len(p)], labels[i, :len(t)] = p, t
        pc[i], lc[i] = len(p), len(t)
    return pred, pc, labels, lc


def ap_case(seed, P_, n_cls=3, niou=10, ties=False):
    """Seeded ap_per_class inputs: P_ predictions of n_cls classes, tp a prefix over the thresholds, at most n_l true
    positives per class, distinct confidences unless `ties`."""
    rng = np.random.default_rng(seed)
    pred_cls = rng.integers(0, n_cls, P_).astype(F)
    n_l = rng.integers(max(1, P_ // (4 * n_cls)), max(2, P_ // n_cls + 2), n_cls)
    level = np.zeros(P_, np.int64)
    for c in range(n_cls):
        idx = np.flatnonzero(pred_cls == c)
        k = min(len(idx), int(n_l[c]), int(rng.integers(0, len(idx) + 1)))
        if k:
            level[rng.choice(idx, k, replace=False)] = rng.integers(1, niou + 1, k)
    tp = (level[:, None] > np.arange(niou)[None, :]).astype(np.uint8)
    if ties:
        conf = (rng.integers(1, 8, P_) / 8.0).astype(F)
    else:
        conf = rng.permutation(P_).astype(np.float64)
        conf = ((conf + rng.uniform(0.1, 0.9, P_)) / (P_ + 1)).astype(F)
        assert len(np.unique(conf)) == P_
    target_cls = np.concatenate([np.full(int(n), c, np.float64) for c, n in enumerate(n_l)])
    return tp, conf, pred_cls, target_cls
