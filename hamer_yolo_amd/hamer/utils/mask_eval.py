"""Mask scores on one HIP call (hm_mask_score, csrc/mask_eval.hip): region similarity J (intersection over union) and contour
accuracy F (boundary precision and recall within a pixel tolerance) of predicted silhouettes against label masks -- the pair
of segmentation measures of the DAVIS benchmark, written from its definition.  The rule is stated in include/hamer_hip.h and
DESIGN.md section 10.2 and is unpinned against DAVIS's own script and skimage, neither of which this project can run.

The predicted silhouette is what ``render.render_views(...)['mesh_id']`` leaves on the device; the masks are the label images
``process_batch_manopara_with_mask`` reads and ``render.hand_maps_folder`` writes.  A query is ``(frame, id_lo, id_hi, label)``:
pred = the pixels whose mesh index lies in [id_lo, id_hi), gt = the pixels whose mask equals ``label`` (-1: any non-zero
label).  One query per frame over all its hands scores masks that carry one hand label; one query per hand with that hand's
own label scores masks that tell the hands apart.  Device tensors in, counts stay on the device.  There is no CPU fallback.

The same masks can correct a hand: ``mask_fit`` (hm_mask_fit, csrc/mask_fit.hip) builds per query the normal equations of a
contour alignment between the predicted silhouette and the mask and solves them for a 2-D similarity, and ``fit_contour`` loops
render, align, move: shift in the image plane, scale (depth) and rotation about the viewing axis.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, Optional, Sequence

import numpy as np
import torch

from ... import lib as L
from .depth_eval import _workspace

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


def _check_pair(who: str, pred_id, mask):
    """The checks both entry points make of the two maps; returns their device and (N, H, W)."""
    if not (torch.is_tensor(pred_id) and torch.is_tensor(mask)):
        raise ValueError(f"{who}: pred_id and mask must be tensors")
    if not (pred_id.is_cuda and mask.is_cuda and pred_id.device == mask.device):
        raise ValueError(f"{who}: pred_id and mask must be on one GPU; there is no CPU path")
    if pred_id.dtype != torch.int32 or mask.dtype != torch.uint8:
        raise ValueError(f"{who}: pred_id must be int32 and mask uint8, got {pred_id.dtype} and {mask.dtype}")
    if pred_id.dim() != 3 or tuple(pred_id.shape) != tuple(mask.shape) or 0 in pred_id.shape:
        raise ValueError(f"{who}: pred_id {tuple(pred_id.shape)} / mask {tuple(mask.shape)}: expected two (N, H, W)")
    if not (pred_id.is_contiguous() and mask.is_contiguous()):
        raise ValueError(f"{who}: pred_id and mask must be contiguous")
    return pred_id.device, tuple(int(v) for v in pred_id.shape)


def mask_counts(pred_id: torch.Tensor, mask: torch.Tensor, queries: Sequence, radius: Optional[int] = None,
                bound_th: float = 0.008, counts: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One hm_mask_score call.  ``pred_id`` (N, H, W) int32 and ``mask`` (N, H, W) uint8, contiguous tensors on one GPU;
    ``queries``: a sequence of (frame, id_lo, id_hi, label); ``radius``: the tolerance in pixels, 0..64 (None:
    ``bound_radius(H, W, bound_th)``).  Returns (Q, 8) int64 on the device (``COUNT_NAMES``), or fills ``counts``.  Enqueued
    on the current stream without synchronising; the workspace is cached per device and stream (``release_workspaces``)."""
    dev, (N, H, W) = _check_pair("mask_counts", pred_id, mask)
    r = bound_radius(H, W, bound_th) if radius is None else int(radius)
    if not 0 <= r <= MAX_RADIUS:
        raise ValueError(f"mask_counts: radius {r} outside 0..{MAX_RADIUS}")
    table = _query_table(queries, N)
    Q = int(table.shape[0])
    if counts is None:
        counts = torch.empty(Q, 8, dtype=torch.int64, device=dev)
    elif not (torch.is_tensor(counts) and counts.device == dev and counts.dtype == torch.int64 and tuple(counts.shape) == (Q, 8)
              and counts.is_contiguous()):
        raise ValueError(f"mask_counts: counts must be a contiguous int64 tensor of shape ({Q}, 8) on {dev}")
    if Q == 0:
        return counts
    lib = L.load()
    with torch.cuda.device(dev):
        stream = L.current_stream()
        ws = _workspace(_ws, dev, stream, int(lib.hm_mask_score_workspace_bytes(Q, H, W, r)))
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


# ---------------------------------------------------------------------------------------------------------------- mask fit
FIT_COUNT_NAMES = ("boundary", "matched", "anchored", "unmatched", "out_of_reach", "reserved5")
MAX_REACH = 4096

_fit_ws: Dict[tuple, torch.Tensor] = {}    # (device index, stream) -> hm_mask_fit's workspace, grown on demand


def release_fit_workspaces() -> None:
    """Drop mask_fit's cached workspaces (the boundary maps of ``mask_counts`` plus 256 bytes per query each)."""
    _fit_ws.clear()


def fit_radius(H: int, W: int) -> int:
    """The search radius of the contour fit in pixels: twice the tolerance of the contour measure, at most 64 -- 36 for
    1080 x 1920, 24 for 720 x 1280."""
    return min(MAX_RADIUS, 2 * bound_radius(H, W))


def _device_table(who: str, rows, dev, width: int, what: str) -> torch.Tensor:
    """``rows`` as a contiguous (Q, width) int32 tensor on ``dev``: a tensor already there is taken as it is (no upload, no
    check of its values), a sequence goes through pinned memory."""
    if torch.is_tensor(rows):
        if not (rows.device == dev and rows.dtype == torch.int32 and rows.dim() == 2 and rows.shape[1] == width and rows.is_contiguous()):
            raise ValueError(f"{who}: a {what} tensor must be contiguous int32 (Q, {width}) on {dev}")
        return rows
    t = np.asarray([tuple(int(v) for v in row) for row in rows], np.int64).reshape(-1, width)
    if t.size and (np.abs(t) >= 2 ** 31).any():
        raise ValueError(f"{who}: a {what} value does not fit int32")
    if not len(t):
        return torch.empty(0, width, dtype=torch.int32, device=dev)
    return torch.from_numpy(np.ascontiguousarray(t.astype(np.int32))).pin_memory().to(dev, non_blocking=True)


def mask_fit(pred_id: torch.Tensor, mask: torch.Tensor, queries, centre, *, radius: int, reach_px: int = MAX_REACH,
             directions: int = 3, damping: float = 1e-3, lever_px: float = 50.0, min_pixels: int = 30) -> Dict[str, torch.Tensor]:
    """One hm_mask_fit call: per query the normal equations of a contour alignment between the predicted silhouette and the
    mask, and their solution for a 2-D similarity about ``centre``.  ``pred_id``, ``mask`` and ``queries`` are
    ``mask_counts``' (a (Q, 4) int32 tensor on the maps' GPU is taken without an upload; a frame outside the batch is then
    legal and gives zeros); ``centre``: (Q, 2) integer pixels (x, y), a sequence or an int32 tensor on that GPU.  A boundary
    pixel is matched with the nearest boundary pixel of the other map within ``radius`` (0..64); ``directions`` 1: pred ->
    mask, 2: mask -> pred, 3: both; a moved point farther than ``reach_px`` (1..4096) from the centre is left out.
    ``damping`` (per used pixel; scale and angle weighted by ``lever_px`` squared) keeps unobserved directions at rest; below
    ``min_pixels`` used pixels a query is not solved.  Returns ``{'sums': (Q, 18) int64, 'counts': (Q, 2, 6) int64 (per
    direction FIT_COUNT_NAMES), 'solution': (Q, 8) float64 (alpha, beta, tx, ty, rms in pixels, solved, 0, 0)}`` on the device:
    the motion is ``q -> centre + (1 + alpha) (q - centre) + beta J (q - centre) + t`` with ``J (x, y) = (-y, x)``.  Enqueued on
    the current stream without synchronising; the workspace is cached per device and stream (``release_fit_workspaces``).
    There is no CPU path."""
    dev, (N, H, W) = _check_pair("mask_fit", pred_id, mask)
    r, reach, directions, min_pixels = int(radius), int(reach_px), int(directions), int(min_pixels)
    if not (0 <= r <= MAX_RADIUS and 1 <= reach <= MAX_REACH and directions in (1, 2, 3) and 0 <= damping < np.inf
            and 0 < lever_px < np.inf and min_pixels >= 1):
        raise ValueError(f"mask_fit: expected radius in 0..{MAX_RADIUS}, reach_px in 1..{MAX_REACH}, directions 1, 2 or 3, "
                         "damping >= 0, lever_px > 0 and min_pixels >= 1")
    qd = _device_table("mask_fit", queries if torch.is_tensor(queries) else _query_table(queries, N), dev, 4, "query")
    cd = _device_table("mask_fit", centre, dev, 2, "centre")
    Q = int(qd.shape[0])
    if int(cd.shape[0]) != Q:
        raise ValueError(f"mask_fit: {int(cd.shape[0])} centres for {Q} queries")
    out = {"sums": torch.empty(Q, 18, dtype=torch.int64, device=dev), "counts": torch.empty(Q, 2, 6, dtype=torch.int64, device=dev),
           "solution": torch.empty(Q, 8, dtype=torch.float64, device=dev)}
    if Q == 0:
        return out
    lib = L.load()
    with torch.cuda.device(dev):
        stream = L.current_stream()
        ws = _workspace(_fit_ws, dev, stream, int(lib.hm_mask_fit_workspace_bytes(Q, H, W, r)))
        L.check(lib.hm_mask_fit(L.ptr(pred_id), L.ptr(mask), N, H, W, L.ptr(qd), Q, L.ptr(cd), r, reach, directions, float(damping),
                                float(lever_px), min_pixels, L.ptr(out["sums"]), L.ptr(out["counts"]), L.ptr(out["solution"]),
                                L.ptr(ws), ws.numel() * 8, stream), "hm_mask_fit")
    return out


def fit_directions(frame_index: Sequence[int], labels: Sequence[int]) -> list:
    """Per hand the directions of its contour fit: 1 (pred -> mask only) for a hand that shares its frame and label with
    another hand -- the mask's contour is then the union of the hands, and the rule cannot tell whose pixel a mask pixel is --
    and 3 (both) for a hand alone under its label."""
    pairs = [(int(f), int(l)) for f, l in zip(frame_index, labels)]
    return [1 if pairs.count(p) > 1 else 3 for p in pairs]


def fit_contour(H: int, W: int, K, vertices: torch.Tensor, faces, cam_t: torch.Tensor, pivot: torch.Tensor,
                frame_index: Sequence[int], mask: torch.Tensor, labels: Sequence[int], rounds: int = 6, *,
                radius: Optional[int] = None, reach_px: int = MAX_REACH, damping: float = 1e-3, lever_px: float = 50.0,
                min_pixels: int = 30, max_rot_rad: float = 0.5, max_scale: float = 2.0, znear: float = 0.05) -> Dict[str, torch.Tensor]:
    """Fit hands to label masks in four degrees of freedom: image-plane shift, scale (depth) and rotation about the viewing
    axis.  ``vertices`` (B, V, 3): the hands' meshes about their origins (MANO's output, left hands mirrored), ``cam_t`` (B, 3):
    the origins in the camera frame, ``pivot`` (B, 3): the point of each hand the similarity is taken about (the wrist joint
    plus ``cam_t`` folds the result into a MANO record), ``frame_index``: per hand the row of ``mask`` (N, H, W) uint8 it
    belongs to, ``labels``: per hand its label in the mask (-1: any non-zero label), ``K`` (3, 3) or (N, 3, 3).  All tensors on
    one GPU.  Per round: ``render_views`` of the placed vertices (mesh_id only), ONE ``mask_fit`` call with one query per hand
    about the pivot's projection rounded to the nearest pixel (two calls when the batch mixes hands that share a label in
    their frame -- fitted pred -> mask only, ``fit_directions`` -- with hands that do not), and on the device, in fp64, with
    s = hypot(1 + alpha, beta) and phi = atan2(beta, 1 + alpha):

        p' = c + (1 + alpha) (p - c) + beta J (p - c) + t   (p: the pivot's real-valued projection, c: the centre)
        pivot' = the point on the ray of p' at depth z / s;   E = exp(phi r),  r the unit ray through the pivot
        R <- E R;   placed <- E (placed - pivot) + pivot'

    for the hands that were solved with |phi| <= ``max_rot_rad``, 1 / ``max_scale`` <= s <= ``max_scale`` and |t| <= radius; a
    hand that was not stays where it is.  Nothing inside the loop synchronises with the host.  Returns ``{'placed': (B, V, 3)
    float64, 'rotation': (B, 3, 3) float64 (the product of the applied steps), 'cam_t': (B, 3) like cam_t (cam_t + pivot' -
    pivot), 'pivot': (B, 3) float64, 'rms': (B,) float64 in pixels and 'pixels': (B,) int64 (matched + anchored) of the last
    round, 'counts': (B, 2, 6) int64 of the last round, 'fitted': (B,) bool}``; a hand that never had a step applied keeps its
    bytes."""
    from ... import render
    from .depth_eval import _cameras, exp_so3
    if not (torch.is_tensor(vertices) and torch.is_tensor(cam_t) and torch.is_tensor(pivot) and torch.is_tensor(mask)
            and vertices.is_cuda and cam_t.device == vertices.device and pivot.device == vertices.device
            and mask.device == vertices.device):
        raise ValueError("fit_contour: vertices, cam_t, pivot and mask must be tensors on one GPU; there is no CPU path")
    B = int(cam_t.shape[0])
    if vertices.dim() != 3 or int(vertices.shape[0]) != B or tuple(cam_t.shape) != (B, 3) or tuple(pivot.shape) != (B, 3) \
            or len(frame_index) != B or len(labels) != B:
        raise ValueError("fit_contour: expected vertices (B, V, 3), cam_t (B, 3), pivot (B, 3), B frame indices and B labels")
    if mask.dim() != 3 or tuple(mask.shape[1:]) != (int(H), int(W)) or mask.dtype != torch.uint8:
        raise ValueError(f"fit_contour: mask must be uint8 (N, {H}, {W}), got {mask.dtype} {tuple(mask.shape)}")
    dev = vertices.device
    N = int(mask.shape[0])
    r = fit_radius(H, W) if radius is None else int(radius)
    faces = torch.as_tensor(faces).to(dev, torch.int32).reshape(-1, 3)
    if faces.numel() and (int(faces.min()) < 0 or int(faces.max()) >= int(vertices.shape[1])):
        raise ValueError(f"fit_contour: face corner outside the {int(vertices.shape[1])} vertices")
    frames = [int(f) for f in frame_index]
    # everything that is uploaded goes up before the first render: the loop below only enqueues
    table = _query_table([(f, j, j + 1, int(l)) for j, (f, l) in enumerate(zip(frames, labels))], N)
    dirs = fit_directions(frames, labels)
    groups = [(d, [j for j in range(B) if dirs[j] == d]) for d in (1, 3)]
    groups = [(d, idx, _device_table("fit_contour", table[idx], dev, 4, "query"),
               None if len(idx) == B else torch.as_tensor(idx, dtype=torch.int64).pin_memory().to(dev, non_blocking=True))
              for d, idx in groups if idx]
    cams = _cameras(K, N, dev)[torch.as_tensor(frames, dtype=torch.int64).pin_memory().to(dev, non_blocking=True)] if B else \
        torch.zeros(0, 4, dtype=torch.float64, device=dev)
    fx, fy, cx, cy = (cams[:, k] for k in range(4))
    cam64 = cam_t.to(torch.float64)
    pv0 = pivot.to(torch.float64)
    pv = pv0
    placed = vertices.to(torch.float64) + cam64[:, None, :]
    R = torch.eye(3, dtype=torch.float64, device=dev)[None].repeat(B, 1, 1)
    fitted = torch.zeros(B, dtype=torch.bool, device=dev)
    rms = torch.zeros(B, dtype=torch.float64, device=dev)
    counts = torch.zeros(B, 2, 6, dtype=torch.int64, device=dev)
    for _ in range(int(rounds) if B else 0):
        meshes = [{"frame": f, "vertices": placed[j], "faces": faces, "faces_checked": True} for j, f in enumerate(frames)]
        mid = render.render_views(H, W, K, meshes, outputs=("mesh_id",), znear=znear, views=N, device=dev)["mesh_id"]
        proj = torch.stack([fx * pv[:, 0] / pv[:, 2] + cx, fy * pv[:, 1] / pv[:, 2] + cy], 1)
        centre = torch.round(proj)
        ci = centre.to(torch.int32).contiguous()
        sol = torch.zeros(B, 8, dtype=torch.float64, device=dev)
        for d, idx, qd, sel in groups:
            s = mask_fit(mid, mask, qd, ci if sel is None else ci[sel].contiguous(), radius=r, reach_px=reach_px, directions=d,
                         damping=damping, lever_px=lever_px, min_pixels=min_pixels)
            if sel is None:
                sol, counts = s["solution"], s["counts"]
            else:
                sol = sol.index_copy(0, sel, s["solution"])
                counts = counts.index_copy(0, sel, s["counts"])
        al, be, t = sol[:, 0], sol[:, 1], sol[:, 2:4]
        sc, phi = torch.hypot(1.0 + al, be), torch.atan2(be, 1.0 + al)
        ok = (sol[:, 5] > 0.5) & (phi.abs() <= float(max_rot_rad)) & (sc >= 1.0 / float(max_scale)) & (sc <= float(max_scale)) \
            & (torch.sqrt((t * t).sum(1)) <= float(r))
        v = proj - centre
        p2 = centre + (1.0 + al)[:, None] * v + be[:, None] * torch.stack([-v[:, 1], v[:, 0]], 1) + t
        z2 = pv[:, 2] / sc
        pv2 = torch.stack([(p2[:, 0] - cx) / fx * z2, (p2[:, 1] - cy) / fy * z2, z2], 1)
        ray = pv / torch.sqrt((pv * pv).sum(1))[:, None]
        E = exp_so3(phi[:, None] * ray)
        moved = torch.einsum("bij,bvj->bvi", E, placed - pv[:, None, :]) + pv2[:, None, :]
        placed = torch.where(ok[:, None, None], moved, placed)
        R = torch.where(ok[:, None, None], E @ R, R)
        pv = torch.where(ok[:, None], pv2, pv)
        fitted = fitted | ok
        rms = sol[:, 4]
    out_t = torch.where(fitted[:, None], (cam64 + (pv - pv0)).to(cam_t.dtype), cam_t)
    pixels = counts[:, :, 1].sum(1) + counts[:, :, 2].sum(1)
    return {"placed": placed, "rotation": R, "cam_t": out_t, "pivot": pv, "rms": rms, "pixels": pixels, "counts": counts,
            "fitted": fitted}
