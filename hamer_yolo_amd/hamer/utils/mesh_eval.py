"""Mesh F-scores and the area under the PCK curve on two HIP kernels (hm_mesh_score, hm_pck_auc; csrc/mesh_eval.hip).

``get_measures``, ``calc_auc`` and ``eval_auc`` carry the names, parameter names and defaults of the reference's
rootnet/KeypointFusion/util/eval_utils.py; the number of keypoints is taken from the data (the reference's fixed 21 is the
K = 21 case).  ``mesh_score`` / ``f_score`` are the F-score of the FreiHAND evaluation -- the shares of each cloud's points
whose nearest point of the other cloud is closer than a threshold, and their harmonic mean -- stated in include/hamer_hip.h
and unpinned against FreiHAND's script (and open3d), neither of which this project can run.  ``MeshEvaluator`` accumulates a
dataset in device buffers, as ``pose_utils.Evaluator`` does.  Device tensors in, nothing copied to the host unless the
reference's return type is numpy.  There is no CPU fallback: without the library or a GPU every call raises
``HipLibraryError``.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from ... import lib as L
from .pose_utils import MAX_POINTS, _device, _f32, pose_eval

MAX_THRESHOLDS = 8
MAX_STEPS = 256
SCORE_OUTPUTS = ("d_pred", "d_gt", "precision", "recall", "fscore", "point_err")


def _bounds(r, n: int, what: str) -> Tuple[int, int]:
    """None (all), a range or (start, stop) -> (start, count)."""
    if r is None:
        return 0, n
    lo, hi = (r.start, r.stop) if isinstance(r, range) else (int(r[0]), int(r[1]))
    if isinstance(r, range) and r.step != 1:
        raise ValueError(f"mesh_score: {what} must be contiguous")
    if not (0 <= lo < hi <= n):
        raise ValueError(f"mesh_score: {what} ({lo}, {hi}) does not lie inside the {n} points")
    return lo, hi - lo


def mesh_score(pred: torch.Tensor, gt: torch.Tensor, root: int = -1, pred_range=None, gt_range=None,
               transform: Optional[torch.Tensor] = None, thresholds: Sequence[float] = (0.005, 0.015),
               want=("fscore", "precision", "recall"), out: Optional[Dict[str, torch.Tensor]] = None) -> Dict[str, torch.Tensor]:
    """One hm_mesh_score launch.  pred (B, P, 3) and gt (B, Q, 3 or 4) fp32 contiguous device tensors, P and Q <= 1024;
    ``root``: index subtracted from every point of both sets first, or -1; ``pred_range`` / ``gt_range``: the participating
    points as (start, stop) or a range (None: all); ``transform`` (B, 13): hm_pose_eval's similarity, applied to pred;
    ``thresholds`` in metres, 8 at the most.  ``want`` names the outputs out of ``d_pred`` (B, n_p), ``d_gt`` (B, n_g),
    ``precision`` / ``recall`` / ``fscore`` (B, T), ``point_err`` (B, n; needs n_p == n_g); ``out`` may hold contiguous fp32
    device tensors of those shapes to fill.  Returns a dict of fp32 device tensors; asynchronous on the current stream."""
    if not (pred.is_cuda and gt.is_cuda):
        raise L.HipLibraryError("libhamer_hip kernels take device tensors; there is no CPU path")
    if pred.dim() != 3 or gt.dim() != 3 or pred.shape[2] != 3 or gt.shape[0] != pred.shape[0] or gt.shape[2] not in (3, 4):
        raise ValueError(f"mesh_score: pred {tuple(pred.shape)} / gt {tuple(gt.shape)}: expected (B, P, 3) and (B, Q, 3 or 4)")
    assert pred.dtype == torch.float32 and gt.dtype == torch.float32 and pred.is_contiguous() and gt.is_contiguous()
    B, P, Q = int(pred.shape[0]), int(pred.shape[1]), int(gt.shape[1])
    if B == 0:
        raise ValueError("mesh_score: empty batch")
    p_lo, n_p = _bounds(pred_range, P, "pred_range")
    g_lo, n_g = _bounds(gt_range, Q, "gt_range")
    thr = [float(t) for t in thresholds]
    if len(thr) > MAX_THRESHOLDS:
        raise ValueError(f"mesh_score: {len(thr)} thresholds, {MAX_THRESHOLDS} at the most")
    if transform is not None:
        assert transform.is_cuda and transform.dtype == torch.float32 and tuple(transform.shape) == (B, 13) and transform.is_contiguous()
    shapes = {"d_pred": (B, n_p), "d_gt": (B, n_g), "precision": (B, len(thr)), "recall": (B, len(thr)),
              "fscore": (B, len(thr)), "point_err": (B, n_p)}
    res: Dict[str, torch.Tensor] = {}
    for name in SCORE_OUTPUTS:
        given = None if out is None else out.get(name)
        if given is not None:
            assert given.is_cuda and given.dtype == torch.float32 and tuple(given.shape) == shapes[name] and given.is_contiguous(), name
            res[name] = given
        elif name in want:
            res[name] = torch.empty(shapes[name], device=pred.device, dtype=torch.float32)
    unknown = [n for n in want if n not in SCORE_OUTPUTS]
    if unknown:
        raise ValueError(f"mesh_score: unknown outputs {unknown}")
    a = L.MeshScoreArgs(pred=L.ptr(pred), gt=L.ptr(gt), transform=L.ptr(transform), B=B, P=P, Q=Q, gt_stride=int(gt.shape[2]),
                        root=int(root), pred_lo=p_lo, pred_n=n_p, gt_lo=g_lo, gt_n=n_g, n_thr=len(thr),
                        thresholds=(C.c_double * 8)(*thr), **{n: L.ptr(res.get(n)) for n in SCORE_OUTPUTS})
    L.check(L.load().hm_mesh_score(C.byref(a), L.current_stream()), "hm_mesh_score")
    return res


def f_score(pred, gt, th: float) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """F-score of pred (B, P, 3) against gt (B, Q, 3) at the distance ``th`` (metres): (fscore, precision, recall), three (B,)
    fp32 device tensors.  precision is the share of pred points within ``th`` of gt, recall the share of gt points within
    ``th`` of pred (FreiHAND's script names them the other way round; F is symmetric)."""
    dev = _device()
    o = mesh_score(_f32(pred, dev), _f32(gt, dev), thresholds=(th,))
    return o["fscore"][:, 0], o["precision"][:, 0], o["recall"][:, 0]


def pck_auc(err: torch.Tensor, val_min: float = 0.0, val_max: float = 0.050, steps: int = 20, chunk_rows: int = 0,
            packed: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
    """One hm_pck_auc call.  err (N, K) fp32 device tensor whose rows are contiguous (a row window or column window of a
    larger buffer is fine).  Returns fp64 device tensors ``pck`` (K, steps), ``auc`` (K,), ``mean_auc`` (1,), ``curve``
    (steps,), ``thresholds`` (steps,); ``packed``: an fp64 device tensor of 1 + 2 * steps to hold the last three, in that
    order.  ``chunk_rows``: samples per workgroup (0: the default); the result does not depend on it."""
    if not err.is_cuda:
        raise L.HipLibraryError("libhamer_hip kernels take device tensors; there is no CPU path")
    if err.dim() != 2 or err.dtype != torch.float32 or (err.shape[1] > 1 and err.stride(1) != 1):
        raise ValueError(f"pck_auc: err must be an (N, K) fp32 tensor with contiguous rows, not {tuple(err.shape)} {err.dtype}")
    N, K, T = int(err.shape[0]), int(err.shape[1]), int(steps)
    if N == 0 or K == 0:
        raise ValueError("pck_auc: no samples (the reference's get_measures fails on an empty list too)")
    ld = int(err.stride(0)) if N > 1 else K
    dev = err.device
    if packed is None:
        packed = torch.empty(1 + 2 * max(T, 0), device=dev, dtype=torch.float64)
    assert packed.is_cuda and packed.dtype == torch.float64 and packed.numel() == 1 + 2 * T and packed.is_contiguous()
    o = {"pck": torch.empty(K, max(T, 0), device=dev, dtype=torch.float64), "auc": torch.empty(K, device=dev, dtype=torch.float64),
         "mean_auc": packed[0:1], "curve": packed[1:1 + T], "thresholds": packed[1 + T:]}
    lib = L.load()
    nbytes = int(lib.hm_pck_auc_workspace_bytes(K, T))
    ws = torch.empty(max(nbytes, 8) // 8, device=dev, dtype=torch.int64)
    a = L.PckAucArgs(err=L.ptr(err), N=N, ld=ld, chunk_rows=int(chunk_rows), val_min=float(val_min), val_max=float(val_max), K=K,
                     steps=T, pck=L.ptr(o["pck"]), auc=L.ptr(o["auc"]), mean_auc=L.ptr(o["mean_auc"]), curve=L.ptr(o["curve"]),
                     thresholds=L.ptr(o["thresholds"]), workspace=L.ptr(ws), workspace_bytes=nbytes)
    L.check(lib.hm_pck_auc(C.byref(a), L.current_stream()), "hm_pck_auc")
    return o


def get_measures(data, val_min=0.0, val_max=0.050, steps=20):
    """eval_utils.py:38-66: the mean area under the PCK curves, the mean curve and the thresholds --
    ``(auc_all, pck_curve_all, thresholds)``, a float and two float64 numpy arrays (one copy).  ``data``: the reference's list
    of per-keypoint lists (``data[k][n]``) or an (N, K) tensor or array; K is taken from it.  Errors are taken as fp32."""
    dev = _device()
    if isinstance(data, (list, tuple)):
        err = _f32(np.asarray(data, np.float32).T, dev)
    else:
        err = _f32(data, dev)
    o = pck_auc(err, val_min, val_max, steps)
    host = torch.cat([o["mean_auc"], o["curve"], o["thresholds"]]).cpu().numpy()
    T = int(steps)
    return float(host[0]), host[1:1 + T].copy(), host[1 + T:].copy()


def _trapz(y, x) -> float:
    y, x = np.asarray(y, np.float64), np.asarray(x, np.float64)
    return float((np.diff(x) * (y[1:] + y[:-1]) / 2.0).sum())


def calc_auc(x, y):
    """eval_utils.py:77-82: the trapezoid area of y over x, divided by that of 1 (host numpy: a dozen values)."""
    return _trapz(y, x) / _trapz(np.ones_like(np.asarray(y, np.float64)), x)


def eval_auc(joint_error_list, sample_number):
    """eval_utils.py:4-35: prints the area under the PCK curve (0-50, 20 steps) and the area between 20 and 50 for stage 0 and
    for stage -1 of ``joint_error_list[i][stage]`` ((n, K) arrays of joint errors, in the unit the thresholds 0..50 are in).
    The reference's quirk is reproduced: its second pass APPENDS the last stage's errors to the first stage's lists, so the
    figures printed under ``stage: -1`` pool both stages.  ``sample_number`` is unused, as in the reference.  K is the width
    of the arrays (the reference reads the first 21 columns)."""
    dev = _device()
    stage = lambda s: torch.cat([_f32(np.asarray(e[s]), dev) for e in joint_error_list])                    # noqa: E731
    first = stage(0)
    for name, err in ((0, first), (-1, None)):
        if err is None:
            err = torch.cat([first, stage(-1)])
        auc, pck_curve_all, threshs = get_measures(err, 0, 50, 20)
        print('stage:', name)
        print('Area under curve: %.3f' % auc)
        pck_curve_all, threshs = pck_curve_all[8:], threshs[8:] * 1000.0
        auc_subset = calc_auc(threshs, pck_curve_all)
        print('Area under curve between 20mm - 50mm: %.3f' % auc_subset)


def _mm_name(th: float) -> str:
    return f"{round(float(th) * 1000.0, 6):g}"


class MeshEvaluator:
    """F-scores of the mesh and the areas under the PCK curves of joints and vertices, raw and Procrustes-aligned, accumulated
    over a dataset in device buffers of ``dataset_length``.  A call takes (B, n_joints + n_verts, 3) point sets, joints first
    (``evaluate._hand_points``); ``root`` is subtracted from every point (-1: nothing).  The aligned figures use the
    similarity of hm_pose_eval on the set they score: joints on joints, vertices on vertices, as FreiHAND aligns each.
    ``thresholds`` (metres) name the F-scores in mm (``f5``, ``f15``, ``pa_f5``, ``pa_f15``); ``auc`` = (val_min, val_max,
    steps) of the PCK curve."""

    def __init__(self, dataset_length: int, n_joints: int = 21, root: int = 0, thresholds: Sequence[float] = (0.005, 0.015),
                 auc: Tuple[float, float, int] = (0.0, 0.05, 100)):
        self.dataset_length = int(dataset_length)
        self.n_joints = int(n_joints)
        self.root = int(root)
        self.thresholds = tuple(float(t) for t in thresholds)
        self.auc = (float(auc[0]), float(auc[1]), int(auc[2]))
        if not 1 <= len(self.thresholds) <= MAX_THRESHOLDS:
            raise ValueError(f"MeshEvaluator: 1..{MAX_THRESHOLDS} thresholds")
        if not 2 <= self.auc[2] <= MAX_STEPS or not self.auc[0] < self.auc[1]:
            raise ValueError(f"MeshEvaluator: auc = (val_min, val_max, steps) with val_min < val_max and steps in 2..{MAX_STEPS}")
        if not 1 <= self.n_joints < MAX_POINTS:
            raise ValueError(f"MeshEvaluator: n_joints in 1..{MAX_POINTS - 1}")
        self.f_names = [f"f{_mm_name(t)}" for t in self.thresholds] + [f"pa_f{_mm_name(t)}" for t in self.thresholds]
        self.counter = 0
        self._buf: Dict[str, torch.Tensor] = {}         # allocated at the first call (the constructor needs no GPU)

    def __call__(self, pred_points, gt_points, sync: bool = False):
        """Score a batch and store it at ``counter``.  Returns the batch's per-hand F-scores by name: (B,) fp32 device tensors
        and no synchronisation with ``sync=False``, numpy arrays (one copy) otherwise."""
        dev = _device()
        P, G = _f32(pred_points, dev), _f32(gt_points, dev)
        if P.dim() != 3 or P.shape != G.shape or P.shape[2] != 3 or not self.n_joints < P.shape[1] <= MAX_POINTS:
            raise ValueError(f"MeshEvaluator: expected two (B, n_joints + n_verts, 3) sets, got {tuple(P.shape)} and {tuple(G.shape)}")
        B, n = int(P.shape[0]), int(P.shape[1])
        if self.counter + B > self.dataset_length:
            raise ValueError(f"MeshEvaluator: {self.counter} + {B} samples exceed dataset_length {self.dataset_length}")
        if not -1 <= self.root < n:
            raise ValueError(f"MeshEvaluator: root {self.root} outside the {n} points")
        nj, nv, T, L_ = self.n_joints, n - self.n_joints, len(self.thresholds), self.dataset_length
        if not self._buf:
            z = lambda w: torch.zeros(L_, w, device=dev, dtype=torch.float32)                              # noqa: E731
            self._buf = {"f": z(T), "pa_f": z(T), "err_j": z(nj), "pa_err_j": z(nj), "err_v": z(nv), "pa_err_v": z(nv)}
        elif self._buf["err_v"].shape[1] != nv:
            raise ValueError(f"MeshEvaluator: {nv} vertices, the earlier batches had {self._buf['err_v'].shape[1]}")
        lo, hi = self.counter, self.counter + B
        w = lambda k: self._buf[k][lo:hi]                                                                  # noqa: E731
        joints, verts = (0, nj), (nj, n)
        tj = pose_eval(P, G, root=self.root, sel=range(*joints), want=("transform",))["transform"]
        tv = pose_eval(P, G, root=self.root, sel=range(*verts), want=("transform",))["transform"]
        kw = dict(root=self.root, thresholds=self.thresholds, want=())
        mesh_score(P, G, pred_range=verts, gt_range=verts, out={"fscore": w("f"), "point_err": w("err_v")}, **kw)
        mesh_score(P, G, pred_range=verts, gt_range=verts, transform=tv, out={"fscore": w("pa_f"), "point_err": w("pa_err_v")}, **kw)
        mesh_score(P, G, pred_range=joints, gt_range=joints, out={"point_err": w("err_j")}, **kw)
        mesh_score(P, G, pred_range=joints, gt_range=joints, transform=tj, out={"point_err": w("pa_err_j")}, **kw)
        self.counter = hi
        both = torch.cat([w("f"), w("pa_f")], 1).t()
        if sync:
            both = both.cpu().numpy()
        return dict(zip(self.f_names, both))

    def per_hand(self) -> Dict[str, np.ndarray]:
        """The F-scores of every hand seen so far, by name: float64 arrays of ``counter`` (one copy)."""
        if self.counter == 0:
            return {k: np.zeros(0) for k in self.f_names}
        both = torch.cat([self._buf["f"][:self.counter], self._buf["pa_f"][:self.counter]], 1).t().double().cpu().numpy()
        return dict(zip(self.f_names, both))

    def result(self) -> Dict[str, float]:
        """The dataset's figures in one copy: the means of the F-scores by name, and ``auc_j``, ``auc_v``, ``pa_auc_j``,
        ``pa_auc_v`` -- hm_pck_auc over the per-point errors of everything seen so far."""
        if self.counter == 0:
            raise ValueError("MeshEvaluator: evaluation has not started")
        c = self.counter
        aucs = [pck_auc(self._buf[k][:c], *self.auc)["mean_auc"] for k in ("err_j", "err_v", "pa_err_j", "pa_err_v")]
        host = torch.cat([self._buf["f"][:c].double().mean(0), self._buf["pa_f"][:c].double().mean(0)] + aucs).cpu().numpy()
        return {k: float(v) for k, v in zip(self.f_names + ["auc_j", "auc_v", "pa_auc_j", "pa_auc_v"], host)}
