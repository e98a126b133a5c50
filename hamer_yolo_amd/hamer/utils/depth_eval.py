"""Hand depth against a sensor depth map on one HIP call (hm_depth_residuals, csrc/depth_eval.hip): per query a histogram of
``sensor - predicted`` over the pixels its meshes cover, six pixel counts, and the lower median, mean, mean absolute value and
rms of the residuals -- and from the median the shift of a hand along its viewing ray (``refine_cam_t``).  The rule is stated
in include/hamer_hip.h ("Depth residuals") and DESIGN.md section 10.3.

The predicted side is what ``render.render_views(..., outputs=('depth', 'mesh_id'))`` leaves on the device; the sensor side is
a batch of 16-bit depth images in raw units (``unit`` metres each, 0 = no measurement) registered to the colour frames.
Device tensors in, results stay on the device.  There is no CPU fallback.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import numpy as np
import torch

from ... import lib as L

MAX_BINS = 4096
COUNT_NAMES = ("covered", "off_mask", "no_measurement", "below", "above", "in_range", "reserved6", "reserved7")

_ws: Dict[tuple, torch.Tensor] = {}        # (device index, stream) -> workspace, grown on demand


def release_workspaces() -> None:
    """Drop the cached workspaces (8 bytes per query each)."""
    _ws.clear()


def _int32_on(who: str, values, dev, n: Optional[int], what: str) -> torch.Tensor:
    if torch.is_tensor(values):
        if not (values.device == dev and values.dtype == torch.int32 and values.dim() == 1 and values.is_contiguous()):
            raise ValueError(f"{who}: a {what} tensor must be contiguous int32 (n,) on {dev}")
        t = values
    else:
        a = np.asarray(values, np.int64).reshape(-1)
        if a.size and (np.abs(a) >= 2 ** 31).any():
            raise ValueError(f"{who}: a {what} value does not fit int32")
        t = torch.from_numpy(np.ascontiguousarray(a.astype(np.int32))).to(dev)
    if n is not None and int(t.shape[0]) != n:
        raise ValueError(f"{who}: {what} has {int(t.shape[0])} entries, expected {n}")
    return t


def _check_maps(who: str, pred_depth, pred_id, sensor, mask, labels, Q: int):
    """What ``depth_residuals`` and ``depth_fit`` (``who``) ask of their maps and of Q; returns the maps' device and (N, H, W)."""
    if not all(torch.is_tensor(t) for t in (pred_depth, pred_id, sensor)):
        raise ValueError(f"{who}: pred_depth, pred_id and sensor must be tensors")
    dev = pred_id.device
    if not (pred_id.is_cuda and pred_depth.device == dev and sensor.device == dev):
        raise ValueError(f"{who}: pred_depth, pred_id and sensor must be on one GPU; there is no CPU path")
    if pred_depth.dtype != torch.float32 or pred_id.dtype != torch.int32 or sensor.dtype not in (torch.uint16, torch.int16):
        raise ValueError(f"{who}: expected float32, int32 and uint16, got {pred_depth.dtype}, {pred_id.dtype}, {sensor.dtype}")
    shape = tuple(pred_id.shape)
    if pred_id.dim() != 3 or 0 in shape or tuple(pred_depth.shape) != shape or tuple(sensor.shape) != shape:
        raise ValueError(f"{who}: pred_depth {tuple(pred_depth.shape)} / pred_id {shape} / sensor {tuple(sensor.shape)}: "
                         "expected three (N, H, W)")
    if not (pred_depth.is_contiguous() and pred_id.is_contiguous() and sensor.is_contiguous()):
        raise ValueError(f"{who}: pred_depth, pred_id and sensor must be contiguous")
    if (mask is None) != (labels is None):
        raise ValueError(f"{who}: mask and labels are given both or neither")
    if mask is not None and not (torch.is_tensor(mask) and mask.device == dev and mask.dtype == torch.uint8
                                 and tuple(mask.shape) == shape and mask.is_contiguous()):
        raise ValueError(f"{who}: mask must be a contiguous uint8 tensor of shape {shape} on {dev}")
    if Q < 0:
        raise ValueError(f"{who}: Q must not be negative")
    return dev, shape


def _labels_on(who: str, labels, dev, Q: int) -> Optional[torch.Tensor]:
    if labels is None:
        return None
    if not torch.is_tensor(labels) and any(not -2 <= int(v) <= 255 for v in np.asarray(labels).reshape(-1)):
        raise ValueError(f"{who}: a label must be -2, -1 or 0..255")
    return _int32_on(who, labels, dev, Q, "labels")


def _workspace(cache: Dict[tuple, torch.Tensor], dev, stream, need: int) -> torch.Tensor:
    """The cached workspace of this device and stream, grown on demand."""
    key = (dev.index if dev.index is not None else torch.cuda.current_device(), stream)
    ws = cache.get(key)
    if ws is None or ws.numel() * 8 < need:
        cache.pop(key, None)
        ws = cache[key] = torch.empty((need + 7) // 8, dtype=torch.int64, device=dev)
    return ws


def depth_residuals(pred_depth: torch.Tensor, pred_id: torch.Tensor, sensor: torch.Tensor, mesh_query, Q: int, *,
                    unit: float = 0.001, bin_m: float = 0.0005, bins: int = 4096, raw_range=(1, 65535),
                    mask: Optional[torch.Tensor] = None, labels=None) -> Dict[str, torch.Tensor]:
    """One hm_depth_residuals call.  ``pred_depth`` (N, H, W) float32, ``pred_id`` (N, H, W) int32 and ``sensor`` (N, H, W)
    uint16 (or int16 holding the same bits), contiguous tensors on one GPU; ``mesh_query``: per mesh row the query its pixels
    count for or -1, a sequence or an int32 tensor on that GPU; ``Q`` queries.  ``unit``: metres per raw unit; ``raw_range``:
    raw values outside it (and 0) are no measurement; ``bin_m`` / ``bins``: the histogram, centred on 0.  ``mask`` (N, H, W)
    uint8 and ``labels`` (per query -2: no test, -1: mask != 0, 0..255: mask == label) restrict the pixels; both or neither.
    Returns ``{'hist': (Q, bins) int32 (the kernel's uint32; a bin holds at most N H W < 2^31), 'counts': (Q, 8) int64
    (COUNT_NAMES), 'stats': (Q, 4) float64 (lower median, mean, mean absolute, rms; NaN where undefined)}`` on the device.  Enqueued on the current stream without
    synchronising; the workspace is cached per device and stream (``release_workspaces``)."""
    Q, bins = int(Q), int(bins)
    dev, (N, H, W) = _check_maps("depth_residuals", pred_depth, pred_id, sensor, mask, labels, Q)
    if bins < 2 or bins > MAX_BINS or bins % 2:
        raise ValueError(f"depth_residuals: bins must be even and in 2..{MAX_BINS}, got {bins}")
    if not (np.isfinite(unit) and unit > 0 and np.isfinite(bin_m) and bin_m > 0):
        raise ValueError("depth_residuals: unit and bin_m must be finite and > 0")
    raw_lo, raw_hi = int(raw_range[0]), int(raw_range[1])
    if raw_lo > raw_hi:
        raise ValueError("depth_residuals: raw_range must be (lo, hi) with lo <= hi")
    mq = _int32_on("depth_residuals", mesh_query, dev, None, "mesh_query")
    lab = _labels_on("depth_residuals", labels, dev, Q)
    out = {"hist": torch.empty(Q, bins, dtype=torch.int32, device=dev), "counts": torch.empty(Q, 8, dtype=torch.int64, device=dev),
           "stats": torch.empty(Q, 4, dtype=torch.float64, device=dev)}
    if Q == 0:
        return out
    lib = L.load()
    with torch.cuda.device(dev):
        stream = L.current_stream()
        ws = _workspace(_ws, dev, stream, int(lib.hm_depth_residuals_workspace_bytes(Q, bins)))
        L.check(lib.hm_depth_residuals(L.ptr(pred_depth), L.ptr(pred_id), L.ptr(sensor), L.ptr(mask), L.ptr(lab), N, H, W,
                                       L.ptr(mq) if mq.numel() else None, int(mq.numel()), Q, float(unit), raw_lo, raw_hi,
                                       float(bin_m), bins, L.ptr(out["hist"]), L.ptr(out["counts"]), L.ptr(out["stats"]),
                                       L.ptr(ws), ws.numel() * 8, stream), "hm_depth_residuals")
    return out


def _host(a, dtype):
    return (a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)).astype(dtype)


def summary_from_hist(hist, counts, bin_m: float, thresholds_m: Sequence[float] = (0.005, 0.010, 0.020)) -> Dict[str, np.ndarray]:
    """Host numpy, from (Q, bins) ``hist`` and (Q, 8) ``counts`` (device tensors -- one copy each -- or arrays).  With valid =
    below + in_range + above, per query: ``median`` (the rule's lower median: the centre of the bin that holds rank
    (valid + 1) // 2, NaN when that rank lies below or above the histogram or valid == 0), ``mean_abs`` (of the bin centres over
    the in-range pixels, NaN without any), ``inliers`` (Q, len(thresholds_m)): the share of the valid pixels whose bin centre c
    has |c| <= t, ``measured`` = valid / covered, ``occluded`` = below / valid (NaN where the denominator is 0), and the integer
    ``valid`` and ``covered``."""
    h = _host(hist, np.int64)
    c = _host(counts, np.int64).reshape(-1, 8)
    Q = len(c)
    h = h.reshape(Q, -1) if Q else np.zeros((0, 0), np.int64)
    bins = h.shape[1]
    centre = ((np.arange(bins) - bins // 2).astype(np.float64) + 0.5) * float(bin_m)
    below, above, inside, covered = c[:, 3], c[:, 4], c[:, 5], c[:, 0]
    valid = below + inside + above
    median = np.full(Q, np.nan)
    mean_abs = np.full(Q, np.nan)
    inliers = np.full((Q, len(thresholds_m)), np.nan)
    for q in range(Q):
        m = (valid[q] + 1) // 2
        if valid[q] > 0 and below[q] < m <= below[q] + inside[q]:
            median[q] = centre[int(np.searchsorted(below[q] + np.cumsum(h[q]), m))]
        nz = np.nonzero(h[q])[0]
        if inside[q] > 0:
            s = 0.0
            for k in nz:
                s = s + float(h[q, k]) * abs(centre[k])
            mean_abs[q] = s / float(inside[q])
        if valid[q] > 0:
            for j, t in enumerate(thresholds_m):
                inliers[q, j] = float(h[q][np.abs(centre) <= float(t)].sum()) / float(valid[q])
    with np.errstate(divide="ignore", invalid="ignore"):
        measured = np.where(covered > 0, valid / np.where(covered > 0, covered, 1), np.nan)
        occluded = np.where(valid > 0, below / np.where(valid > 0, valid, 1), np.nan)
    return {"median": median, "mean_abs": mean_abs, "inliers": inliers, "measured": measured.astype(np.float64),
            "occluded": occluded.astype(np.float64), "valid": valid, "covered": covered}


class DepthEvaluator:
    """Depth residuals over a dataset: every call scores a batch's queries and keeps their histograms and counts on the
    device; nothing is copied until ``per_query`` / ``result``.  The histogram (``unit``, ``bin_m``, ``bins``, ``raw_range``)
    is fixed at construction so that all rows are comparable."""

    def __init__(self, unit: float = 0.001, bin_m: float = 0.0005, bins: int = 4096, raw_range=(1, 65535),
                 thresholds_m: Sequence[float] = (0.005, 0.010, 0.020)):
        self.unit, self.bin_m, self.bins, self.raw_range = float(unit), float(bin_m), int(bins), tuple(raw_range)
        self.thresholds_m = tuple(float(t) for t in thresholds_m)
        self._hist, self._counts = [], []
        self.n = 0

    def __call__(self, pred_depth, pred_id, sensor, mesh_query, Q, sync: bool = False, mask=None, labels=None):
        """Score and append.  Returns the batch's ``depth_residuals`` dict: device tensors and no synchronisation with
        ``sync=False``, numpy arrays (one copy each) otherwise."""
        r = depth_residuals(pred_depth, pred_id, sensor, mesh_query, Q, unit=self.unit, bin_m=self.bin_m, bins=self.bins,
                            raw_range=self.raw_range, mask=mask, labels=labels)
        self._hist.append(r["hist"])
        self._counts.append(r["counts"])
        self.n += int(Q)
        return {k: v.cpu().numpy() for k, v in r.items()} if sync else r

    def hist(self) -> np.ndarray:
        """(n, bins) int64 histograms of every query seen so far, in call order (one copy)."""
        if not self._hist:
            return np.zeros((0, self.bins), np.int64)
        return torch.cat(self._hist).cpu().numpy().astype(np.int64)

    def counts(self) -> np.ndarray:
        """(n, 8) int64 counts of every query seen so far, in call order (one copy)."""
        if not self._counts:
            return np.zeros((0, 8), np.int64)
        return torch.cat(self._counts).cpu().numpy()

    def per_query(self) -> Dict[str, np.ndarray]:
        """``summary_from_hist`` of every query seen so far."""
        return summary_from_hist(self.hist(), self.counts(), self.bin_m, self.thresholds_m)

    def result(self) -> Dict:
        """The dataset summary: ``hands`` (queries seen), ``scored`` (those with a finite median), ``median_abs_mm`` (the
        median over the scored hands of |median residual|) and ``mean_abs_mm`` (the mean over them of the mean absolute
        residual), in millimetres; ``inliers`` (per threshold the share of ALL valid pixels within it), ``measured`` (valid /
        covered) and ``occluded`` (below / valid) pooled over all hands' pixels.  NaN where nothing was scored."""
        if self.n == 0:
            raise ValueError("DepthEvaluator: evaluation has not started")
        return dataset_summary(self.hist(), self.counts(), self.bin_m, self.thresholds_m)


def dataset_summary(hist, counts, bin_m: float, thresholds_m: Sequence[float] = (0.005, 0.010, 0.020)) -> Dict:
    """``DepthEvaluator.result`` of given (n, bins) histograms and (n, 8) counts."""
    s = summary_from_hist(hist, counts, bin_m, thresholds_m)
    ok = np.isfinite(s["median"])
    nan = float("nan")
    valid, covered = int(s["valid"].sum()), int(s["covered"].sum())
    inl = [nan] * len(thresholds_m)
    if valid:
        w = s["valid"].astype(np.float64)
        inl = [float(np.nansum(s["inliers"][:, j] * w) / valid) for j in range(len(thresholds_m))]
    below = int(_host(counts, np.int64).reshape(-1, 8)[:, 3].sum())
    return {"hands": int(len(ok)), "scored": int(ok.sum()),
            "median_abs_mm": float(np.median(np.abs(s["median"][ok])) * 1000.0) if ok.any() else nan,
            "mean_abs_mm": float(np.mean(s["mean_abs"][ok]) * 1000.0) if ok.any() else nan,
            "inliers": {f"{t * 1000.0:g}mm": v for t, v in zip(thresholds_m, inl)},
            "measured": valid / covered if covered else nan, "occluded": below / valid if valid else nan}


def _renderer(who: str, H: int, W: int, K, vertices: torch.Tensor, faces, frame_index: Sequence[int], znear: float, N: int):
    """``faces`` as int32 on the vertices' device, checked against them once, before any loop; and ``draw(placed)``: the
    ``render_views`` depth and mesh_id maps of one mesh per hand, ``placed[j]`` in frame ``frame_index[j]`` of N."""
    from ... import render
    dev = vertices.device
    faces = torch.as_tensor(faces).to(dev, torch.int32).reshape(-1, 3)
    if faces.numel() and (int(faces.min()) < 0 or int(faces.max()) >= int(vertices.shape[1])):
        raise ValueError(f"{who}: face corner outside the {int(vertices.shape[1])} vertices")

    def draw(placed):
        meshes = [{"frame": int(f), "vertices": placed[j], "faces": faces, "faces_checked": True} for j, f in enumerate(frame_index)]
        return render.render_views(H, W, K, meshes, outputs=("depth", "mesh_id"), znear=znear, views=N, device=dev)
    return faces, draw


def refine_cam_t(H: int, W: int, K, vertices: torch.Tensor, faces, cam_t: torch.Tensor, frame_index: Sequence[int],
                 sensor: torch.Tensor, *, unit: float, iterations: int = 2, min_pixels: int = 200, min_fraction: float = 0.25,
                 znear: float = 0.05, mask: Optional[torch.Tensor] = None, labels=None, bin_m: float = 0.0005, bins: int = 4096,
                 raw_range=(1, 65535)) -> Dict[str, torch.Tensor]:
    """Move hands along the rays of their origins until their rendered depth agrees with the sensor's.  ``vertices``
    (B, V, 3): the hands' meshes about their origins (MANO's output, left hands mirrored), ``cam_t`` (B, 3): the origins in
    the camera frame, ``frame_index``: per hand the row of ``sensor`` (N, H, W) uint16 it belongs to, ``K`` (3, 3) or
    (N, 3, 3), ``faces`` (F, 3).  All tensors on one GPU.  Per iteration: ``render_views`` of ``vertices + cam_t`` (depth and
    mesh_id), one ``depth_residuals`` call with one query per hand, and

        cam_t' = cam_t * ((tz + median) / tz)        (fp64, rounded once to cam_t's dtype)

    for the hands whose median is finite, whose valid pixels (below + in range + above) are >= ``min_pixels`` and >=
    ``min_fraction`` of the covered ones, and for which tz + median > ``znear``.  Scaling cam_t moves the origin along its own
    ray: its pixel stays where it was.  This is NOT ``custom_cam_crop_to_full(depth_refine=...)``, which re-derives tx and ty
    from the crop camera the records do not keep.  Nothing inside the loop synchronises with the
    host.  Returns ``{'cam_t': (B, 3) like cam_t, 'median': (B,) float64 of the last iteration, 'valid': (B,) int64 of the last
    iteration, 'updated': (B,) bool}``; a hand that was never updated keeps its bytes."""
    if not (torch.is_tensor(vertices) and torch.is_tensor(cam_t) and vertices.is_cuda and cam_t.device == vertices.device):
        raise ValueError("refine_cam_t: vertices and cam_t must be tensors on one GPU; there is no CPU path")
    B = int(cam_t.shape[0])
    if vertices.dim() != 3 or int(vertices.shape[0]) != B or tuple(cam_t.shape) != (B, 3) or len(frame_index) != B:
        raise ValueError("refine_cam_t: expected vertices (B, V, 3), cam_t (B, 3) and B frame indices")
    dev = vertices.device
    faces, draw = _renderer("refine_cam_t", H, W, K, vertices, faces, frame_index, znear, int(sensor.shape[0]))
    query = torch.arange(B, dtype=torch.int32, device=dev)
    lab = None if labels is None else _int32_on("depth_residuals", labels, dev, B, "labels")
    cur = cam_t.clone()
    updated = torch.zeros(B, dtype=torch.bool, device=dev)
    median = torch.full((B,), float("nan"), dtype=torch.float64, device=dev)
    valid = torch.zeros(B, dtype=torch.int64, device=dev)
    for _ in range(int(iterations)):
        r = draw(vertices + cur[:, None, :].to(vertices.dtype))
        s = depth_residuals(r["depth"], r["mesh_id"], sensor, query, B, unit=unit, bin_m=bin_m, bins=bins, raw_range=raw_range,
                            mask=mask, labels=lab)
        c = s["counts"]
        median, valid = s["stats"][:, 0], c[:, 3] + c[:, 4] + c[:, 5]
        tz = cur[:, 2].to(torch.float64)
        ok = torch.isfinite(median) & (valid >= int(min_pixels)) & \
            (valid.to(torch.float64) / c[:, 0].to(torch.float64) >= float(min_fraction)) & (tz + median > float(znear))
        moved = (cur.to(torch.float64) * ((tz + median) / tz)[:, None]).to(cur.dtype)
        cur = torch.where(ok[:, None], moved, cur)
        updated = updated | ok
    return {"cam_t": cur, "median": median, "valid": valid, "updated": updated}


# ---------------------------------------------------------------------------------------------------------------- depth fit
FIT_COUNT_NAMES = ("covered", "off_mask", "no_measurement", "gated", "no_normal", "rejected", "used", "reserved7")

_fit_ws: Dict[tuple, torch.Tensor] = {}    # (device index, stream) -> hm_depth_fit's workspace, grown on demand


def release_fit_workspaces() -> None:
    """Drop depth_fit's cached workspaces (288 bytes per query each)."""
    _fit_ws.clear()


def _cameras(K, N: int, dev) -> torch.Tensor:
    """(N, 4) float64 fx, fy, cx, cy on ``dev`` of K (3, 3) or (N, 3, 3), an array or a tensor (a device tensor is not copied
    to the host)."""
    Kt = K.to(dev, torch.float64) if torch.is_tensor(K) else torch.from_numpy(np.asarray(K, np.float64)).to(dev)
    if tuple(Kt.shape) == (3, 3):
        Kt = Kt[None].expand(N, 3, 3)
    if tuple(Kt.shape) != (N, 3, 3):
        raise ValueError(f"depth_fit: K must be (3, 3) or ({N}, 3, 3), got {tuple(Kt.shape)}")
    return torch.stack([Kt[:, 0, 0], Kt[:, 1, 1], Kt[:, 0, 2], Kt[:, 1, 2]], 1).contiguous()


def depth_fit(pred_depth: torch.Tensor, pred_id: torch.Tensor, sensor: torch.Tensor, mesh_query, Q: int, K, pivot: torch.Tensor, *,
              unit: float, gate_m: float = 0.03, edge_m: float = 0.005, reach_m: float = 0.5, damping: float = 1e-3,
              lever_m: float = 0.05, min_pixels: int = 200, raw_range=(1, 65535), mask: Optional[torch.Tensor] = None,
              labels=None) -> Dict[str, torch.Tensor]:
    """One hm_depth_fit call: per query the normal equations of a point-to-plane fit of the predicted surface to the sensor's,
    and their solution.  The maps, ``mesh_query``, ``Q``, ``unit``, ``raw_range``, ``mask`` and ``labels`` are
    ``depth_residuals``'; ``K`` (3, 3) or (N, 3, 3); ``pivot`` (Q, 3) float64 on the maps' GPU: the point each query's rotation
    turns about.  A pixel takes part when its residual is within ``gate_m``, its four neighbours belong to the same mesh within
    ``edge_m`` of its depth, and it lies within ``reach_m`` of the pivot.  ``damping`` (per used pixel; rotations weighted by
    ``lever_m`` squared) keeps unobserved directions at rest; below ``min_pixels`` used pixels a query is not solved.
    Returns ``{'sums': (Q, 28) int64, 'counts': (Q, 8) int64 (FIT_COUNT_NAMES), 'solution': (Q, 8) float64 (omega, t, rms,
    solved)}`` on the device: the motion is ``p -> p + omega x (p - pivot) + t``.  Enqueued on the current stream without
    synchronising; the workspace is cached per device and stream (``release_fit_workspaces``).  There is no CPU path."""
    return _depth_fit(pred_depth, pred_id, sensor, mesh_query, Q, K, pivot, unit=unit, gate_m=gate_m, edge_m=edge_m,
                      reach_m=reach_m, damping=damping, lever_m=lever_m, min_pixels=min_pixels, raw_range=raw_range, mask=mask,
                      labels=labels)


def _depth_fit(pred_depth, pred_id, sensor, mesh_query, Q, cameras, pivot, *, unit, gate_m, edge_m, reach_m, damping, lever_m,
               min_pixels, raw_range, mask, labels):
    """``depth_fit`` with ``cameras`` either its ``K`` or what ``_cameras`` made of one: (N, 4) float64 on the maps' GPU."""
    Q, min_pixels = int(Q), int(min_pixels)
    dev, (N, H, W) = _check_maps("depth_fit", pred_depth, pred_id, sensor, mask, labels, Q)
    if not (np.isfinite(unit) and unit > 0):
        raise ValueError("depth_fit: unit must be finite and > 0")
    if not (0 < gate_m <= 0.25 and 0 < edge_m < np.inf and 0 < reach_m <= 1 and 0 <= damping < np.inf and 0 < lever_m < np.inf
            and min_pixels >= 1):
        raise ValueError("depth_fit: expected gate_m in (0, 0.25], edge_m > 0, reach_m in (0, 1], damping >= 0, lever_m > 0 "
                         "and min_pixels >= 1")
    raw_lo, raw_hi = int(raw_range[0]), int(raw_range[1])
    if raw_lo > raw_hi:
        raise ValueError("depth_fit: raw_range must be (lo, hi) with lo <= hi")
    if not (torch.is_tensor(pivot) and pivot.device == dev and pivot.dtype == torch.float64 and tuple(pivot.shape) == (Q, 3)
            and pivot.is_contiguous()):
        raise ValueError(f"depth_fit: pivot must be a contiguous float64 tensor of shape ({Q}, 3) on {dev}")
    made = torch.is_tensor(cameras) and tuple(cameras.shape) == (N, 4) and cameras.dtype == torch.float64 \
        and cameras.device == dev and cameras.is_contiguous()
    cams = cameras if made else _cameras(cameras, N, dev)
    mq = _int32_on("depth_fit", mesh_query, dev, None, "mesh_query")
    lab = _labels_on("depth_fit", labels, dev, Q)
    out = {"sums": torch.empty(Q, 28, dtype=torch.int64, device=dev), "counts": torch.empty(Q, 8, dtype=torch.int64, device=dev),
           "solution": torch.empty(Q, 8, dtype=torch.float64, device=dev)}
    if Q == 0:
        return out
    lib = L.load()
    with torch.cuda.device(dev):
        stream = L.current_stream()
        ws = _workspace(_fit_ws, dev, stream, int(lib.hm_depth_fit_workspace_bytes(Q)))
        L.check(lib.hm_depth_fit(L.ptr(pred_depth), L.ptr(pred_id), L.ptr(sensor), L.ptr(mask), L.ptr(lab), N, H, W,
                                 L.ptr(mq) if mq.numel() else None, int(mq.numel()), Q, L.ptr(cams), L.ptr(pivot), float(unit),
                                 raw_lo, raw_hi, float(gate_m), float(edge_m), float(reach_m), float(damping), float(lever_m),
                                 min_pixels, L.ptr(out["sums"]), L.ptr(out["counts"]), L.ptr(out["solution"]), L.ptr(ws),
                                 ws.numel() * 8, stream), "hm_depth_fit")
    return out


def exp_so3(omega: torch.Tensor) -> torch.Tensor:
    """Rodrigues' formula on the device, fp64: (B, 3) rotation vectors -> (B, 3, 3); the series below 1e-8 rad."""
    w = omega.to(torch.float64)
    th = torch.sqrt((w * w).sum(-1))[:, None, None]
    z = torch.zeros_like(w[:, 0])
    Kx = torch.stack([torch.stack([z, -w[:, 2], w[:, 1]], -1), torch.stack([w[:, 2], z, -w[:, 0]], -1),
                      torch.stack([-w[:, 1], w[:, 0], z], -1)], -2)
    small = th < 1e-8
    ths = torch.where(small, torch.ones_like(th), th)
    a = torch.where(small, 1.0 - th * th / 6.0, torch.sin(ths) / ths)
    b = torch.where(small, 0.5 - th * th / 24.0, (1.0 - torch.cos(ths)) / (ths * ths))
    return torch.eye(3, dtype=torch.float64, device=w.device) + a * Kx + b * (Kx @ Kx)


def fit_rigid(H: int, W: int, K, vertices: torch.Tensor, faces, cam_t: torch.Tensor, pivot: torch.Tensor,
              frame_index: Sequence[int], sensor: torch.Tensor, *, unit: float, ray_iterations: int = 2, iterations: int = 6,
              max_rot_rad: float = 0.5, max_shift_m: float = 0.1, gate_m: float = 0.03, edge_m: float = 0.005,
              reach_m: float = 0.5, damping: float = 1e-3, lever_m: float = 0.05, min_pixels: int = 200, min_fraction: float = 0.25,
              znear: float = 0.05, mask: Optional[torch.Tensor] = None, labels=None, bin_m: float = 0.0005, bins: int = 4096,
              raw_range=(1, 65535)) -> Dict[str, torch.Tensor]:
    """Fit hands rigidly -- all six degrees of freedom -- to the sensor's depth.  Arguments as ``refine_cam_t``, and ``pivot``
    (B, 3): the point of each hand, in the camera frame, its rotation turns about (the wrist joint plus ``cam_t`` folds the
    result into a MANO record).  First ``ray_iterations`` rounds of ``refine_cam_t`` bring the hands inside the gate (the
    pivot moves with its hand); then per iteration ``render_views`` of the placed vertices (depth and mesh_id), ONE
    ``depth_fit`` call with one query per hand, and on the device, in fp64,

        R <- exp(omega) R;   placed <- exp(omega) (placed - pivot) + pivot + t;   pivot <- pivot + t

    for the hands that were solved with |omega| <= ``max_rot_rad`` and |t| <= ``max_shift_m``.  Nothing inside the loops
    synchronises with the host.  Returns ``{'rotation': (B, 3, 3) float64 (the product of the applied steps), 'cam_t': (B, 3)
    like cam_t (the ray rounds' plus the sum of the applied t), 'pivot': (B, 3) float64, 'placed': (B, V, 3) float64 (the fitted
    vertices: rotation (vertices + ray cam_t - ray pivot) + pivot), 'rms': (B,) float64 and 'used': (B,) int64 of the last
    iteration, 'updated': (B,) bool (a ray or a rigid step was applied), 'fitted': (B,) bool (a rigid step was), 'median' and
    'valid': the ray rounds' last (NaN and 0 without any)}``; a hand that never had a step applied keeps its bytes."""
    if not (torch.is_tensor(vertices) and torch.is_tensor(cam_t) and torch.is_tensor(pivot) and vertices.is_cuda
            and cam_t.device == vertices.device and pivot.device == vertices.device):
        raise ValueError("fit_rigid: vertices, cam_t and pivot must be tensors on one GPU; there is no CPU path")
    B = int(cam_t.shape[0])
    if vertices.dim() != 3 or int(vertices.shape[0]) != B or tuple(cam_t.shape) != (B, 3) or tuple(pivot.shape) != (B, 3) \
            or len(frame_index) != B:
        raise ValueError("fit_rigid: expected vertices (B, V, 3), cam_t (B, 3), pivot (B, 3) and B frame indices")
    dev = vertices.device
    N = int(sensor.shape[0])
    faces, draw = _renderer("fit_rigid", H, W, K, vertices, faces, frame_index, znear, N)
    cams = _cameras(K, N, dev)
    if int(ray_iterations) > 0:
        ray = refine_cam_t(H, W, K, vertices, faces, cam_t, frame_index, sensor, unit=unit, iterations=int(ray_iterations),
                           min_pixels=min_pixels, min_fraction=min_fraction, znear=znear, mask=mask, labels=labels, bin_m=bin_m,
                           bins=bins, raw_range=raw_range)
        cam_ray, updated, median, valid = ray["cam_t"], ray["updated"], ray["median"], ray["valid"]
    else:
        cam_ray, updated = cam_t, torch.zeros(B, dtype=torch.bool, device=dev)
        median = torch.full((B,), float("nan"), dtype=torch.float64, device=dev)
        valid = torch.zeros(B, dtype=torch.int64, device=dev)
    cam64 = cam_ray.to(torch.float64)
    pv = (pivot.to(torch.float64) + (cam64 - cam_t.to(torch.float64))).contiguous()
    placed = vertices.to(torch.float64) + cam64[:, None, :]
    query = torch.arange(B, dtype=torch.int32, device=dev)
    lab = None if labels is None else _int32_on("depth_fit", labels, dev, B, "labels")
    R = torch.eye(3, dtype=torch.float64, device=dev)[None].repeat(B, 1, 1)
    shift = torch.zeros(B, 3, dtype=torch.float64, device=dev)
    fitted = torch.zeros(B, dtype=torch.bool, device=dev)
    rms = torch.full((B,), float("nan"), dtype=torch.float64, device=dev)
    used = torch.zeros(B, dtype=torch.int64, device=dev)
    for _ in range(int(iterations)):
        r = draw(placed)
        s = _depth_fit(r["depth"], r["mesh_id"], sensor, query, B, cams, pv, unit=unit, gate_m=gate_m, edge_m=edge_m, reach_m=reach_m,
                       damping=damping, lever_m=lever_m, min_pixels=min_pixels, raw_range=raw_range, mask=mask, labels=lab)
        sol = s["solution"]
        w, t = sol[:, :3], sol[:, 3:6]
        ok = (sol[:, 7] > 0.5) & (torch.sqrt((w * w).sum(1)) <= float(max_rot_rad)) & (torch.sqrt((t * t).sum(1)) <= float(max_shift_m))
        E = exp_so3(w)
        moved = torch.einsum("bij,bvj->bvi", E, placed - pv[:, None, :]) + pv[:, None, :] + t[:, None, :]
        placed = torch.where(ok[:, None, None], moved, placed)
        R = torch.where(ok[:, None, None], E @ R, R)
        step = torch.where(ok[:, None], t, torch.zeros_like(t))
        shift = shift + step
        pv = (pv + step).contiguous()
        fitted = fitted | ok
        rms, used = sol[:, 6], s["counts"][:, 6]
    out_t = torch.where(fitted[:, None], (cam64 + shift).to(cam_t.dtype), cam_ray)
    return {"rotation": R, "cam_t": out_t, "pivot": pv, "placed": placed, "rms": rms, "used": used,
            "updated": updated | fitted, "fitted": fitted, "median": median, "valid": valid}
