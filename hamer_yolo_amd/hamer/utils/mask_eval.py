"""Mask scores on one HIP call (hm_mask_score, csrc/mask_eval.hip): region similarity J (intersection over union) and contour
accuracy F (boundary precision and recall within a pixel tolerance) of predicted silhouettes against label masks -- the pair
of segmentation measures of the DAVIS benchmark, written from its definition.  The rule is stated in include/hamer_hip.h and
DESIGN.md section 10.2 and is unpinned against DAVIS's own script and skimage, neither of which this project can run.

The predicted silhouette is what ``render.render_views(...)['mesh_id']`` leaves on the device; the masks are the label images
``process_batch_manopara_with_mask`` reads and ``render.hand_maps_folder`` writes.  A query is ``(frame, id_lo, id_hi, label)``:
pred = the pixels whose mesh index lies in [id_lo, id_hi), gt = the pixels whose mask equals ``label`` (-1: any non-zero
label).  One query per frame over all its hands scores masks that carry one hand label; one query per hand with that hand's
own label scores masks that tell the hands apart.  Device tensors in, counts stay on the device.  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, Optional, Sequence

import numpy as np
import torch

from ... import lib as L

MAX_RADIUS = 64
COUNT_NAMES = ("inter", "pred_area", "gt_area", "pred_boundary", "gt_boundary", "pred_matched", "gt_matched", "pixels")

_ws: Dict[tuple, torch.Tensor] = {}        # (device index, stream) -> workspace, grown on demand


def release_workspaces() -> None:
    """Drop the cached boundary-map workspaces (Q * 2 * H * ceil(W / 64) * 8 bytes each: 0.5 MB per 1080p query)."""
    _ws.clear()


def bound_radius(H: int, W: int, bound_th: float = 0.008) -> int:
    """The tolerance of the contour measure in pixels: ``bound_th`` itself when it is >= 1, else
    ceil(bound_th * sqrt(H^2 + W^2)) -- 18 for 1080 x 1920, 12 for 720 x 1280."""
    if bound_th >= 1:
        return int(bound_th)
    return int(math.ceil(bound_th * math.sqrt(float(H) * H + float(W) * W)))


def _query_table(queries, N: int) -> np.ndarray:
    q = np.asarray([tuple(int(v) for v in row) for row in queries], np.int64).reshape(-1, 4)
    if q.size and (np.abs(q) >= 2 ** 31).any():
        raise ValueError("mask_counts: a query value does not fit int32")
    bad = [int(f) for f in q[:, 0] if not 0 <= f < N]
    if bad:
        raise ValueError(f"mask_counts: query frame {bad[0]} outside the batch of {N}")
    return np.ascontiguousarray(q.astype(np.int32))


def mask_counts(pred_id: torch.Tensor, mask: torch.Tensor, queries: Sequence, radius: Optional[int] = None,
                bound_th: float = 0.008, counts: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One hm_mask_score call.  ``pred_id`` (N, H, W) int32 and ``mask`` (N, H, W) uint8, contiguous tensors on one GPU;
    ``queries``: a sequence of (frame, id_lo, id_hi, label); ``radius``: the tolerance in pixels, 0..64 (None:
    ``bound_radius(H, W, bound_th)``).  Returns (Q, 8) int64 on the device (``COUNT_NAMES``), or fills ``counts``.  Enqueued
    on the current stream without synchronising; the workspace is cached per device and stream (``release_workspaces``)."""
    if not (torch.is_tensor(pred_id) and torch.is_tensor(mask)):
        raise ValueError("mask_counts: pred_id and mask must be tensors")
    if not (pred_id.is_cuda and mask.is_cuda and pred_id.device == mask.device):
        raise ValueError("mask_counts: pred_id and mask must be on one GPU; there is no CPU path")
    if pred_id.dtype != torch.int32 or mask.dtype != torch.uint8:
        raise ValueError(f"mask_counts: pred_id must be int32 and mask uint8, got {pred_id.dtype} and {mask.dtype}")
    if pred_id.dim() != 3 or tuple(pred_id.shape) != tuple(mask.shape) or 0 in pred_id.shape:
        raise ValueError(f"mask_counts: pred_id {tuple(pred_id.shape)} / mask {tuple(mask.shape)}: expected two (N, H, W)")
    if not (pred_id.is_contiguous() and mask.is_contiguous()):
        raise ValueError("mask_counts: pred_id and mask must be contiguous")
    N, H, W = (int(v) for v in pred_id.shape)
    r = bound_radius(H, W, bound_th) if radius is None else int(radius)
    if not 0 <= r <= MAX_RADIUS:
        raise ValueError(f"mask_counts: radius {r} outside 0..{MAX_RADIUS}")
    table = _query_table(queries, N)
    Q, dev = int(table.shape[0]), pred_id.device
    if counts is None:
        counts = torch.empty(Q, 8, dtype=torch.int64, device=dev)
    elif not (torch.is_tensor(counts) and counts.device == dev and counts.dtype == torch.int64 and tuple(counts.shape) == (Q, 8)
              and counts.is_contiguous()):
        raise ValueError(f"mask_counts: counts must be a contiguous int64 tensor of shape ({Q}, 8) on {dev}")
    if Q == 0:
        return counts
    lib = L.load()
    need = int(lib.hm_mask_score_workspace_bytes(Q, H, W, r))
    with torch.cuda.device(dev):
        stream = L.current_stream()
        key = (dev.index if dev.index is not None else torch.cuda.current_device(), stream)
        ws = _ws.get(key)
        if ws is None or ws.numel() * 8 < need:
            _ws.pop(key, None)
            ws = _ws[key] = torch.empty((need + 7) // 8, dtype=torch.int64, device=dev)
        qd = torch.from_numpy(table).to(dev)
        L.check(lib.hm_mask_score(L.ptr(pred_id), L.ptr(mask), N, H, W, L.ptr(qd), Q, r, L.ptr(counts), L.ptr(ws), ws.numel() * 8,
                                  stream), "hm_mask_score")
    return counts


def box_query_table(queries) -> np.ndarray:
    """``queries``, a sequence of (frame, label), as the (Q, 2) int32 table hm_mask_boxes reads.  A frame outside the batch is
    legal there (its row is the empty one), so nothing but the int32 range is checked."""
    q = np.asarray([tuple(int(v) for v in row) for row in queries], np.int64).reshape(-1, 2)
    if q.size and (np.abs(q) >= 2 ** 31).any():
        raise ValueError("mask_boxes: a query value does not fit int32")
    return np.ascontiguousarray(q.astype(np.int32))


def mask_boxes(mask: torch.Tensor, queries, boxes: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One hm_mask_boxes call (csrc/mask_boxes.hip): the tight box and the pixel count of a label per query.  ``mask``
    (N, H, W) uint8, a contiguous tensor on a GPU; ``queries``: a sequence of (frame, label) -- label -1: any non-zero label --
    or a (Q, 2) int32 tensor already on the mask's device (no upload then).  Returns (Q, 5) int32 on the device, or fills
    ``boxes``: x1, y1, x2, y2, count, and -1, -1, -1, -1, 0 where the label is absent or the frame outside the batch.
    Enqueued on the current stream without synchronising.  There is no CPU path."""
    if not torch.is_tensor(mask) or not mask.is_cuda:
        raise ValueError("mask_boxes: mask must be a tensor on a GPU; there is no CPU path")
    if mask.dtype != torch.uint8 or mask.dim() != 3 or 0 in mask.shape or not mask.is_contiguous():
        raise ValueError(f"mask_boxes: mask must be a contiguous uint8 (N, H, W) tensor, got {mask.dtype} {tuple(mask.shape)}")
    N, H, W = (int(v) for v in mask.shape)
    dev = mask.device
    if torch.is_tensor(queries):
        if not (queries.device == dev and queries.dtype == torch.int32 and queries.dim() == 2 and queries.shape[1] == 2
                and queries.is_contiguous()):
            raise ValueError(f"mask_boxes: a query tensor must be contiguous int32 (Q, 2) on {dev}")
        qd = queries
    else:
        table = box_query_table(queries)
        qd = torch.from_numpy(table).pin_memory().to(dev, non_blocking=True) if len(table) else torch.empty(0, 2, dtype=torch.int32, device=dev)
    Q = int(qd.shape[0])
    if boxes is None:
        boxes = torch.empty(Q, 5, dtype=torch.int32, device=dev)
    elif not (torch.is_tensor(boxes) and boxes.device == dev and boxes.dtype == torch.int32 and tuple(boxes.shape) == (Q, 5)
              and boxes.is_contiguous()):
        raise ValueError(f"mask_boxes: boxes must be a contiguous int32 tensor of shape ({Q}, 5) on {dev}")
    if Q == 0:
        return boxes
    with torch.cuda.device(dev):
        L.check(L.load().hm_mask_boxes(L.ptr(mask), N, H, W, L.ptr(qd), Q, L.ptr(boxes), L.current_stream()), "hm_mask_boxes")
    return boxes


def jf_from_counts(counts) -> Dict[str, np.ndarray]:
    """``J``, ``F``, ``precision`` and ``recall`` of (Q, 8) counts (a device tensor -- one copy -- or a numpy array) as float64
    arrays, by the rule: J = 1 when both areas are empty, else inter / union; P = pred_matched / pred_boundary and R =
    gt_matched / gt_boundary, with P = R = 1 when neither boundary exists, P = 1, R = 0 when only gt has one and P = 0, R = 1
    when only pred has one; F = 0 when P + R == 0, else 2 P R / (P + R)."""
    c = counts.cpu().numpy() if torch.is_tensor(counts) else np.asarray(counts)
    c = c.astype(np.int64).reshape(-1, 8)
    inter, pa, ga, pb, gb, pm, gm = (c[:, k] for k in range(7))
    union = pa + ga - inter
    one = np.ones(len(c), np.float64)
    J = np.where(pa + ga == 0, one, inter / np.where(union == 0, 1, union))
    P = np.where(pb == 0, one, np.where(gb == 0, 0.0, pm / np.where(pb == 0, 1, pb)))
    R = np.where(gb == 0, one, np.where(pb == 0, 0.0, gm / np.where(gb == 0, 1, gb)))
    s = P + R
    F = np.where(s == 0, 0.0, 2 * P * R / np.where(s == 0, 1.0, s))
    return {"J": J.astype(np.float64), "F": F.astype(np.float64), "precision": P.astype(np.float64), "recall": R.astype(np.float64)}


class MaskEvaluator:
    """J and F over a dataset: every call scores a batch's queries and keeps their counts on the device; nothing is copied
    until ``per_query`` / ``result``."""

    def __init__(self):
        self._rows = []
        self.n = 0

    def __call__(self, pred_id, mask, queries, sync: bool = False, radius: Optional[int] = None, bound_th: float = 0.008):
        """Score and append.  Returns the batch's (Q, 8) counts: the device tensor and no synchronisation with ``sync=False``,
        a numpy array (one copy) otherwise."""
        c = mask_counts(pred_id, mask, queries, radius=radius, bound_th=bound_th)
        self._rows.append(c)
        self.n += int(c.shape[0])
        return c.cpu().numpy() if sync else c

    def counts(self) -> np.ndarray:
        """(n, 8) int64 counts of every query seen so far, in call order (one copy)."""
        if not self._rows:
            return np.zeros((0, 8), np.int64)
        return torch.cat(self._rows).cpu().numpy()

    def per_query(self) -> Dict[str, np.ndarray]:
        """``J``, ``F``, ``precision``, ``recall`` of every query seen so far: float64 arrays of ``n``."""
        return jf_from_counts(self.counts())

    def result(self) -> Dict[str, float]:
        """``j_mean``, ``j_recall`` (the share of queries with J > 0.5), ``f_mean``, ``f_recall`` (the same for F),
        ``jf_mean`` = (j_mean + f_mean) / 2 and ``n``."""
        if self.n == 0:
            raise ValueError("MaskEvaluator: evaluation has not started")
        s = self.per_query()
        j_mean, f_mean = float(s["J"].mean()), float(s["F"].mean())
        return {"j_mean": j_mean, "j_recall": float((s["J"] > 0.5).mean()), "f_mean": f_mean,
                "f_recall": float((s["F"] > 0.5).mean()), "jf_mean": (j_mean + f_mean) / 2.0, "n": int(self.n)}
