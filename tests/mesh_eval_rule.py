"""The rules hm_mesh_score and hm_pck_auc are tested against, in numpy fp64.

mesh_score: per hand, the root subtraction and (optionally) the similarity transform of pose_eval_rule.apply_transform, the
nearest-neighbour distance of every participating point of one set to the other set, both ways, the shares below each
threshold (strict <) and F = 2 p r / (p + r), 0 when p + r == 0 -- the F-score of the FreiHAND evaluation, unpinned against
FreiHAND's script and open3d: this statement is the definition.  get_measures: get_measures / _get_pck / calc_auc of the
reference's rootnet/KeypointFusion/util/eval_utils.py (:38-82) with the number of keypoints taken from the data (the
reference's fixed 21 is the K = 21 case).  Inputs are taken as they are given (fp32) and widened; nothing here rounds."""
import numpy as np

import pose_eval_rule as PR


def _trapz(y, x):
    """np.trapz (removed from numpy 2.x under that name): sum of d * (y[1:] + y[:-1]) / 2."""
    y, x = np.asarray(y, np.float64), np.asarray(x, np.float64)
    return (np.diff(x) * (y[1:] + y[:-1]) / 2.0).sum()


def mesh_score(pred, gt, root=-1, pred_range=None, gt_range=None, transform=None, thresholds=(0.005, 0.015)):
    """pred (B, P, 3), gt (B, Q, 3 or 4); ranges (start, stop) or None (all) -> dict: d_pred (B, n_p), d_gt (B, n_g), n_pred / n_gt
    (B, T) integer counts below each threshold, precision, recall, fscore (B, T), point_err (B, n) when n_p == n_g."""
    pred = np.asarray(pred, np.float64)
    gt = np.asarray(gt, np.float64)[:, :, :3]
    p_lo, p_hi = (0, pred.shape[1]) if pred_range is None else pred_range
    g_lo, g_hi = (0, gt.shape[1]) if gt_range is None else gt_range
    n_p, n_g = p_hi - p_lo, g_hi - g_lo
    if root >= 0:
        gt = gt - gt[:, [root]]
    if transform is not None:
        x = PR.apply_transform(pred, transform, root=root, sel=range(p_lo, p_lo + n_p))
    else:
        x = (pred - pred[:, [root]] if root >= 0 else pred)[:, p_lo:p_lo + n_p]
    y = gt[:, g_lo:g_lo + n_g]
    d = x[:, :, None, :] - y[:, None, :, :]
    with np.errstate(invalid="ignore"):
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        d_pred, d_gt = np.sqrt(d2.min(2)), np.sqrt(d2.min(1))                  # numpy.min hands a NaN on
        thr = np.asarray(thresholds, np.float64)
        n_pred, n_gt = (d_pred[:, :, None] < thr).sum(1), (d_gt[:, :, None] < thr).sum(1)
    p, r = n_pred / n_p, n_gt / n_g
    with np.errstate(invalid="ignore", divide="ignore"):
        f = np.where(p + r == 0.0, 0.0, 2.0 * p * r / (p + r))
    out = {"d_pred": d_pred, "d_gt": d_gt, "n_pred": n_pred, "n_gt": n_gt, "precision": p, "recall": r, "fscore": f}
    if n_p == n_g:
        e = x - y
        out["point_err"] = np.sqrt((e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2])
    return out


def threshold_margin(rule, thresholds):
    """The smallest relative distance of any of the rule's finite distances to any threshold."""
    d = np.concatenate([rule["d_pred"].ravel(), rule["d_gt"].ravel()])
    d = d[np.isfinite(d)]
    return min(float((np.abs(d - t) / t).min()) for t in thresholds) if d.size else np.inf


def get_measures(data, val_min=0.0, val_max=0.050, steps=20):
    """data: (N, K) array or the reference's list of K per-keypoint lists -> (auc_all, pck_curve_all (T,), thresholds (T,),
    pck (K, T), auc (K,))."""
    err = np.asarray(data, np.float64)
    if isinstance(data, (list, tuple)):
        err = err.T                                                            # the reference's data[k][n]
    thresholds = np.linspace(val_min, val_max, steps)
    norm = _trapz(np.ones_like(thresholds), thresholds)
    with np.errstate(invalid="ignore"):
        pck = np.stack([[np.mean((err[:, k] <= t).astype('float')) for t in thresholds] for k in range(err.shape[1])])
    auc = np.array([_trapz(c, thresholds) / norm for c in pck])
    return float(np.mean(auc)), np.mean(pck, 0), thresholds, pck, auc


def get_measures_sorted(err, val_min=0.0, val_max=0.050, steps=20):
    """get_measures for large (N, K) arrays: #(err <= t) is read off each keypoint's sorted errors (NaN sorts last and is never
    counted), an integer, and divided by N once -- the bits of the mean of 0 / 1.  tests/test_mesh_eval_host.py holds it equal
    to get_measures.  -> the same five values."""
    err = np.asarray(err, np.float64)
    thresholds = np.linspace(val_min, val_max, steps)
    norm = _trapz(np.ones_like(thresholds), thresholds)
    s = np.sort(err, axis=0)
    pck = np.stack([np.searchsorted(s[:, k], thresholds, side="right") for k in range(err.shape[1])]) / float(err.shape[0])
    auc = np.array([_trapz(c, thresholds) / norm for c in pck])
    return float(np.mean(auc)), np.mean(pck, 0), thresholds, pck, auc


def calc_auc(x, y):
    return _trapz(y, x) / _trapz(np.ones_like(np.asarray(y, np.float64)), x)


def torch_f_score(pred, gt, thresholds):
    """The F-score chain in torch ops on the tensors' device (what tools/bench_mesh_eval.py times the kernel against): an fp64
    broadcast distance matrix, two minima, the comparisons.  pred (B, P, 3), gt (B, Q, 3) -> fscore (B, T) fp64."""
    import torch
    d = pred.double()[:, :, None, :] - gt.double()[:, None, :, :]
    d2 = (d * d).sum(-1)
    d_pred, d_gt = d2.min(2).values.sqrt(), d2.min(1).values.sqrt()
    thr = torch.as_tensor(thresholds, dtype=torch.float64, device=pred.device)
    p = (d_pred[:, :, None] < thr).double().mean(1)
    r = (d_gt[:, :, None] < thr).double().mean(1)
    return torch.where(p + r == 0, torch.zeros_like(p), 2 * p * r / (p + r))


def torch_auc(err, val_min, val_max, steps):
    """The AUC chain in torch ops: (err[..., None] <= thr).double().mean(0) plus trapezoids -> (mean auc, curve (T,))."""
    import torch
    thr = torch.linspace(val_min, val_max, steps, dtype=torch.float64, device=err.device)
    pck = (err.double()[..., None] <= thr).double().mean(0)
    auc = torch.trapezoid(pck, thr) / torch.trapezoid(torch.ones_like(thr), thr)
    return auc.mean(), pck.mean(0)
