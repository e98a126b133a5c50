"""The rule hm_pose_eval is tested against: hamer/utils/pose_utils.py restated in numpy fp64 -- the similarity Procrustes of
compute_similarity_transform (:9-58), reconstruction_error (:60-71), the means of eval_pose (:73-87), the root subtraction and
keypoint selection of Evaluator.__call__ (:163-168) -- plus the same chain in torch ops on device tensors (what
tools/bench_pose_eval.py times the kernel against) and the PCK rule of EvaluatorPCK (mmpose's keypoint_pck_accuracy with
normalize = 1, restated; unpinned against mmpose).  Inputs are taken as they are given (fp32) and widened; nothing here rounds."""
import numpy as np


def similarity_transform(S1, S2):
    """(B, N, 3) x 2 -> S1_hat (B, N, 3), scale (B,), R (B, 3, 3), t (B, 3), sign (B,) = sign det(U V^T), sigma (B, 3); fp64.
    var1 == 0 gives NaN in S1_hat, scale and t, as the reference's 0 / 0 does."""
    S1 = np.asarray(S1, np.float64).transpose(0, 2, 1)
    S2 = np.asarray(S2, np.float64).transpose(0, 2, 1)
    mu1, mu2 = S1.mean(2, keepdims=True), S2.mean(2, keepdims=True)
    X1, X2 = S1 - mu1, S2 - mu2
    var1 = (X1 ** 2).sum((1, 2))
    K = X1 @ X2.transpose(0, 2, 1)
    U, s, Vh = np.linalg.svd(K)                               # K = U diag(s) Vh; torch.svd's V is Vh^T
    V = Vh.transpose(0, 2, 1)
    sign = np.sign(np.linalg.det(U @ Vh))
    Z = np.tile(np.eye(3), (len(K), 1, 1))
    Z[:, 2, 2] *= sign
    R = V @ Z @ U.transpose(0, 2, 1)
    with np.errstate(invalid="ignore", divide="ignore"):
        scale = np.trace(R @ K, axis1=1, axis2=2) / var1
        t = mu2 - scale[:, None, None] * (R @ mu1)
        S1_hat = scale[:, None, None] * (R @ S1) + t
    return S1_hat.transpose(0, 2, 1), scale, R, t[:, :, 0], sign, s


def pose_eval(pred, gt, root=-1, sel=None):
    """hm_pose_eval in fp64.  pred (B, P, 3), gt (B, P, 3 or 4); root: index or -1; sel: ascending indices or None (all).
    -> dict err (B,), pa_err (B,), aligned (B, n_sel, 3), transform (B, 13) = scale, R row-major, t."""
    pred = np.asarray(pred, np.float64)
    gt = np.asarray(gt, np.float64)[:, :, :3]
    if root >= 0:
        pred = pred - pred[:, [root]]
        gt = gt - gt[:, [root]]
    if sel is not None:
        sel = sorted(int(i) for i in sel)
        pred, gt = pred[:, sel], gt[:, sel]
    err = np.sqrt(((pred - gt) ** 2).sum(-1)).mean(-1)
    hat, scale, R, t, _, _ = similarity_transform(pred, gt)
    pa = np.sqrt(((hat - gt) ** 2).sum(-1)).mean(-1)
    var1 = ((pred - pred.mean(1, keepdims=True)) ** 2).sum((1, 2))
    R = np.where((var1 == 0)[:, None, None], np.nan, R)      # the kernel reports the whole transform of such a hand as NaN
    return {"err": err, "pa_err": pa, "aligned": hat, "transform": np.concatenate([scale[:, None], R.reshape(-1, 9), t], 1)}


def apply_transform(pred, transform, root=-1, sel=None):
    """scale * R * x + t in fp64 on the root-subtracted, selected points of pred."""
    pred = np.asarray(pred, np.float64)
    if root >= 0:
        pred = pred - pred[:, [root]]
    if sel is not None:
        pred = pred[:, sorted(int(i) for i in sel)]
    tr = np.asarray(transform, np.float64)
    return tr[:, None, 0:1] * (pred @ tr[:, 1:10].reshape(-1, 3, 3).transpose(0, 2, 1)) + tr[:, None, 10:13]


def sel_words(sel, P):
    """Indices -> the 16 uint64 words of hm_pose_eval_args.sel (None -> all zero = all points)."""
    words = [0] * 16
    for i in ([] if sel is None else sel):
        words[int(i) >> 6] |= 1 << (int(i) & 63)
    return words


def torch_chain(pred, gt):
    """The reference's computation with torch ops on the tensors' device (torch.linalg.svd for the deprecated torch.svd):
    (mpjpe, pa_mpjpe) as (B,) tensors, no host copy."""
    import torch
    mpjpe = torch.sqrt(((pred - gt) ** 2).sum(-1)).mean(-1)
    S1, S2 = pred.permute(0, 2, 1), gt.permute(0, 2, 1)
    mu1, mu2 = S1.mean(2, keepdim=True), S2.mean(2, keepdim=True)
    X1, X2 = S1 - mu1, S2 - mu2
    var1 = (X1 ** 2).sum(dim=(1, 2))
    K = X1 @ X2.permute(0, 2, 1)
    U, _, Vh = torch.linalg.svd(K)
    V = Vh.permute(0, 2, 1)
    Z = torch.eye(3, device=K.device).unsqueeze(0).repeat(K.shape[0], 1, 1)
    Z[:, -1, -1] *= torch.sign(torch.linalg.det(U @ Vh))
    R = V @ Z @ U.permute(0, 2, 1)
    scale = ((R @ K).diagonal(dim1=-1, dim2=-2).sum(-1) / var1)[:, None, None]
    t = mu2 - scale * (R @ mu1)
    hat = (scale * (R @ S1) + t).permute(0, 2, 1)
    return mpjpe, torch.sqrt(((hat - gt) ** 2).sum(-1)).mean(-1)


def pck(pred, gt, mask, thr):
    """keypoint_pck_accuracy(pred (N, K, 2), gt (N, K, 2), mask (N, K) bool, thr, normalize = 1) -> acc (K,), avg_acc, cnt.
    d[n, k] = |pred - gt| where the mask holds, invalid elsewhere; acc[k] = share of the valid samples of keypoint k with
    d < thr, -1 when it has none; avg_acc = mean of the acc[k] >= 0 (0 when there is none); cnt = how many those are."""
    pred, gt, mask = np.asarray(pred, np.float64), np.asarray(gt, np.float64), np.asarray(mask, bool)
    d = np.sqrt(((pred - gt) ** 2).sum(-1))
    acc = np.full(pred.shape[1], -1.0)
    for k in range(pred.shape[1]):
        if mask[:, k].any():
            acc[k] = float((d[mask[:, k], k] < thr).mean())
    valid = acc[acc >= 0]
    return acc, (float(valid.mean()) if len(valid) else 0.0), int(len(valid))
