"""Hands across frames (csrc/motion.hip; the rule is stated in include/hamer_hip.h, "Motion", and DESIGN.md section 10.8): the
frame-to-frame acceleration of point tracks (``track_jitter``), a zero-phase filter that averages rotations as rotations and
fills frames the detector missed (``track_smooth``), and the host code that turns a folder's records into tracks and back
(``natural_key``, ``sequence_tracks``, ``smooth_hands``, ``summary``).

A record is ``{'right': hand or None, 'left': hand or None}`` per frame, so a track is one side over the sorted frames: nothing
is associated.  ``track_smooth`` and ``track_jitter`` take and return device tensors and never synchronise; there is no CPU
path.  The default radius (4 frames) and sigma (2 frames) are choices, not measurements, and so is the default ``max_fill`` of
the drivers (2: a gap is filled only from neighbours at most two frames away).
"""
from __future__ import annotations

import ctypes as C
import re
from typing import Dict, List, Optional, Sequence

import numpy as np

STATUSES = ("KEPT", "SMOOTHED", "FILLED", "ABSENT", "DEGENERATE")
KEPT, SMOOTHED, FILLED, ABSENT, DEGENERATE = range(5)
MAX_RADIUS = 32
MAX_POINTS = 1024
RADIUS, SIGMA, MAX_FILL = 4, 2.0, 2        # choices, not measurements (module docstring)
SIDES = ("right", "left")
POSE_KEYS = ("pose_global", "pose_hand", "theta", "betas", "cam_t")


def window_weights(radius: int, sigma: float) -> np.ndarray:
    """The window of ``track_smooth``, (radius + 1,) float64 on the host: w[0] = 1, w[k] = exp(-0.5 (k / sigma)^2).  The only
    place the weights are made: the kernel takes them as data."""
    if int(radius) != radius or not 0 <= int(radius) <= MAX_RADIUS:
        raise ValueError(f"track_smooth: the radius must be an integer in 0..{MAX_RADIUS}, got {radius}")
    if not (np.isfinite(sigma) and sigma > 0):
        raise ValueError(f"track_smooth: sigma must be finite and > 0, got {sigma}")
    k = np.arange(int(radius) + 1, dtype=np.float64)
    w = np.exp(-0.5 * (k / float(sigma)) ** 2)
    w[0] = 1.0
    return w


def _device_tensor(t, name: str, what: str):
    import torch
    if not (torch.is_tensor(t) and t.is_cuda):
        raise ValueError(f"{what}: {name} must be a tensor on a GPU; there is no CPU path")
    return t


def _presence(present, shape, dev, what: str):
    import torch
    if not (torch.is_tensor(present) and present.is_cuda and present.device == dev):
        raise ValueError(f"{what}: present must be a tensor on the GPU of the data; there is no CPU path")
    if tuple(present.shape) != tuple(shape):
        raise ValueError(f"{what}: present must be {tuple(shape)}, got {tuple(present.shape)}")
    return present


def track_smooth(rot, lin, present, radius: int = RADIUS, sigma: float = SIGMA, stream=None, weights=None) -> Dict[str, object]:
    """One hm_track_smooth call.  ``rot`` (N, S, J, 3, 3) rotation matrices, ``lin`` (N, S, C) linear channels, ``present``
    (N, S) (non-zero: the hand is there), all on one GPU; N frames, S tracks.  Frame t of a track becomes the weighted mean of
    itself (if present) and of every PAIR t - k, t + k, k <= radius, that lies in the sequence with both ends present -- the
    rotations as the rotation nearest the mean matrix (12 Newton steps of the polar iteration, no trigonometry).  Returns
    device tensors ``rot`` (N, S, J, 3, 3) and ``lin`` (N, S, C) float64, ``status`` (``STATUSES``), ``pairs`` and
    ``nearest_pair`` (N, S) int32 and ``moved`` (N, S, J) float64, the squared Frobenius distance of a SMOOTHED rotation from
    its input (``moved_degrees``), NaN otherwise.  KEPT and DEGENERATE hands keep their input's bytes; ABSENT ones are NaN.
    ``weights`` overrides ``window_weights(radius, sigma)``.  Enqueued on ``stream`` (default: the current one)."""
    import torch
    from ... import lib as L
    w = window_weights(radius, sigma) if weights is None else np.ascontiguousarray(weights, np.float64)
    if not (w.ndim == 1 and 1 <= len(w) <= MAX_RADIUS + 1):
        raise ValueError(f"track_smooth: the radius must be an integer in 0..{MAX_RADIUS}")
    rot, lin = _device_tensor(rot, "rot", "track_smooth"), _device_tensor(lin, "lin", "track_smooth")
    if rot.dim() != 5 or tuple(rot.shape[3:]) != (3, 3) or lin.dim() != 3 or tuple(lin.shape[:2]) != tuple(rot.shape[:2]) or lin.device != rot.device:
        raise ValueError(f"track_smooth: rot must be (N, S, J, 3, 3) and lin (N, S, C) on one GPU, got {tuple(rot.shape)} and {tuple(lin.shape)}")
    N, S, J = (int(v) for v in rot.shape[:3])
    Cn = int(lin.shape[2])
    dev = rot.device
    present = _presence(present, (N, S), dev, "track_smooth")
    with torch.cuda.stream(stream) if stream is not None else torch.cuda.device(dev):
        r, ln = rot.to(torch.float64).contiguous(), lin.to(torch.float64).contiguous()
        here = (present != 0).to(torch.uint8)
        out = {"rot": torch.empty_like(r), "lin": torch.empty_like(ln),
               "status": torch.empty(N, S, dtype=torch.int32, device=dev), "pairs": torch.empty(N, S, dtype=torch.int32, device=dev),
               "nearest_pair": torch.empty(N, S, dtype=torch.int32, device=dev), "moved": torch.empty(N, S, J, dtype=torch.float64, device=dev)}
        if N and S:
            p = lambda t: L.ptr(t) if t.numel() else None                 # noqa: E731
            L.check(L.load().hm_track_smooth(p(r), p(ln), L.ptr(here), N, S, J, Cn, w.ctypes.data_as(C.POINTER(C.c_double)), len(w) - 1,
                                             p(out["rot"]), p(out["lin"]), L.ptr(out["status"]), L.ptr(out["pairs"]),
                                             L.ptr(out["nearest_pair"]), p(out["moved"]), L.current_stream()), "hm_track_smooth")
    return out


def track_jitter(points, present, stream=None):
    """One hm_track_jitter call.  ``points`` (N, S, P, 3) and ``present`` (N, S) on one GPU, P <= 1024.  Returns ``accel``
    (N, S) float64 on the device: the mean over the points of |x[t-1] - 2 x[t] + x[t+1]|, in the points' unit per frame^2,
    where the three frames are present; NaN elsewhere (the two ends, and next to an absent frame)."""
    import torch
    from ... import lib as L
    points = _device_tensor(points, "points", "track_jitter")
    if points.dim() != 4 or points.shape[3] != 3:
        raise ValueError(f"track_jitter: points must be (N, S, P, 3), got {tuple(points.shape)}")
    N, S, P = (int(v) for v in points.shape[:3])
    if P > MAX_POINTS:
        raise ValueError(f"track_jitter: at most {MAX_POINTS} points, got {P}")
    dev = points.device
    present = _presence(present, (N, S), dev, "track_jitter")
    with torch.cuda.stream(stream) if stream is not None else torch.cuda.device(dev):
        x = points.to(torch.float64).contiguous()
        here = (present != 0).to(torch.uint8)
        accel = torch.empty(N, S, dtype=torch.float64, device=dev)
        if N and S:
            L.check(L.load().hm_track_jitter(L.ptr(x) if P else None, L.ptr(here), N, S, P, L.ptr(accel), L.current_stream()),
                    "hm_track_jitter")
    return accel


def moved_degrees(moved):
    """The angle in degrees between a rotation and its smoothed version from ``moved``, their squared Frobenius distance
    8 sin^2(angle / 2) (numpy array or tensor -> numpy float64; NaN stays NaN)."""
    m = np.asarray(moved.cpu() if hasattr(moved, "cpu") else moved, np.float64)
    with np.errstate(invalid="ignore"):
        return np.degrees(2.0 * np.arcsin(np.sqrt(np.clip(m / 8.0, 0.0, 1.0))))


def natural_key(stem: str):
    """Sort key under which runs of digits compare as integers: ``frame_2`` before ``frame_10``.  Host only."""
    return [(0, int(p), "") if p.isdigit() else (1, 0, p) for p in re.split(r"(\d+)", stem) if p != ""]


def sequence_tracks(records: Sequence[dict]) -> Dict[str, np.ndarray]:
    """Sorted record dicts -> the tracks of the two sides, host numpy: ``present`` (N, 2) uint8, ``axis_angle`` (N, 2, 16, 3)
    float64 (``pose_global`` then the 15 of ``pose_hand``) and ``lin`` (N, 2, 13) float64 (``cam_t`` then ``betas``); an absent
    side is zeros.  ``track_hand`` is the way back."""
    N = len(records)
    present = np.zeros((N, 2), np.uint8)
    aa = np.zeros((N, 2, 16, 3), np.float64)
    lin = np.zeros((N, 2, 13), np.float64)
    for t, rec in enumerate(records):
        for s, side in enumerate(SIDES):
            h = rec.get(side) if rec is not None else None
            if h is None:
                continue
            present[t, s] = 1
            aa[t, s, 0] = np.asarray(h["pose_global"], np.float64).reshape(3)
            aa[t, s, 1:] = np.asarray(h["pose_hand"], np.float64).reshape(15, 3)
            lin[t, s, :3] = np.asarray(h["cam_t"], np.float64).reshape(3)
            lin[t, s, 3:] = np.asarray(h["betas"], np.float64).reshape(10)
    return {"present": present, "axis_angle": aa, "lin": lin}


def track_hand(axis_angle, lin, like: Optional[dict] = None) -> Dict[str, np.ndarray]:
    """The five pose keys of one hand from its track row, ``axis_angle`` (16, 3) and ``lin`` (13,), in the dtypes and shapes
    of the hand ``like`` (default: what ``infer.hand_record`` writes: float32, flat)."""
    aa = np.asarray(axis_angle, np.float64).reshape(16, 3)
    ln = np.asarray(lin, np.float64).reshape(13)
    values = {"pose_global": aa[0], "pose_hand": aa[1:], "theta": aa, "betas": ln[3:], "cam_t": ln[:3]}
    out = {}
    for k, v in values.items():
        ref = np.asarray(like[k]) if like is not None and k in like else None
        out[k] = v.reshape(ref.shape).astype(ref.dtype) if ref is not None else v.reshape(-1).astype(np.float32)
    return out


def smooth_tracks(tracks: Dict[str, np.ndarray], device, radius: int = RADIUS, sigma: float = SIGMA) -> Dict[str, np.ndarray]:
    """``sequence_tracks``'s arrays -> matrices (``infer.axis_angle_to_rotation_matrix_torch``, fp64 on the device) ->
    ``track_smooth`` -> axis-angle (``infer.rodrigues_log_batch``).  Returns host numpy: ``status``, ``pairs``, ``nearest_pair``
    (N, 2) int32, ``moved_deg`` (N, 2, 16) float32, ``axis_angle`` (N, 2, 16, 3) float32 and ``lin`` (N, 2, 13) float64.  One
    copy each way.  (The drivers patch this function's name to test their record folding without a GPU.)"""
    import torch
    from ...infer import axis_angle_to_rotation_matrix_torch, rodrigues_log_batch
    N = len(tracks["present"])
    aa = torch.from_numpy(np.ascontiguousarray(tracks["axis_angle"], np.float64)).to(device)
    rot = axis_angle_to_rotation_matrix_torch(aa.reshape(-1, 3)).reshape(N, 2, 16, 3, 3)
    r = track_smooth(rot, torch.from_numpy(np.ascontiguousarray(tracks["lin"], np.float64)).to(device),
                     torch.from_numpy(np.ascontiguousarray(tracks["present"], np.uint8)).to(device), radius, sigma)
    host = {k: v.cpu().numpy() for k, v in r.items()}
    filtered = (host["status"] == SMOOTHED) | (host["status"] == FILLED)
    out_aa = np.zeros((N, 2, 16, 3), np.float32)
    if filtered.any():
        out_aa[filtered] = rodrigues_log_batch(host["rot"][filtered].reshape(-1, 3, 3)).reshape(-1, 16, 3)
    return {"status": host["status"], "pairs": host["pairs"], "nearest_pair": host["nearest_pair"],
            "moved_deg": moved_degrees(host["moved"]).astype(np.float32), "axis_angle": out_aa, "lin": host["lin"]}


def fold_hand(hand: Optional[dict], is_right: bool, status: int, pairs: int, nearest_pair: int, axis_angle, lin, moved_deg,
              max_fill: int = MAX_FILL) -> Optional[dict]:
    """One side of one record after smoothing (host only).  SMOOTHED: new pose keys in the old dtypes and shapes, the old ones
    under ``*_unsmoothed``, ``track_status``, ``track_pairs``, ``track_moved_deg`` (16 float32).  KEPT or DEGENERATE: every
    byte of the pose keys stays, ``track_status`` and ``track_pairs`` are added.  Absent: filled when FILLED and
    ``nearest_pair <= max_fill`` -- the five pose keys, ``is_right``, ``track_status``, ``track_pairs``, ``track_filled``, nothing
    else -- and None otherwise."""
    status = int(status)
    if hand is None:
        if status != FILLED or not 0 < int(nearest_pair) <= int(max_fill):
            return None
        out = track_hand(axis_angle, lin)
        out.update(is_right=bool(is_right), track_status=STATUSES[status], track_pairs=int(pairs), track_filled=True)
        return out
    out = dict(hand)
    if status == SMOOTHED:
        for k in ("pose_global", "pose_hand", "betas", "cam_t"):
            out[k + "_unsmoothed"] = hand[k]
        out.update(track_hand(axis_angle, lin, like=hand))
        out["track_moved_deg"] = np.asarray(moved_deg, np.float32).reshape(16)
    out["track_status"], out["track_pairs"] = STATUSES[status], int(pairs)
    return out


def smooth_hands(hamer, records: Sequence[dict], radius: int = RADIUS, sigma: float = SIGMA, max_fill: int = MAX_FILL) -> List[dict]:
    """The records of a sequence, sorted, smoothed: records -> ``sequence_tracks`` -> ``smooth_tracks`` on ``hamer.device`` ->
    ``fold_hand`` per side.  Returns new record dicts; keys other than 'right' and 'left' keep their objects."""
    if int(max_fill) < 0:
        raise ValueError("smooth_hands: max_fill must be >= 0")
    tracks = sequence_tracks(records)
    r = smooth_tracks(tracks, hamer.device, radius, sigma) if len(records) else None
    out = []
    for t, rec in enumerate(records):
        new = dict(rec)
        for s, side in enumerate(SIDES):
            new[side] = fold_hand(rec.get(side), side == "right", r["status"][t, s], r["pairs"][t, s], r["nearest_pair"][t, s],
                                  r["axis_angle"][t, s], r["lin"][t, s], r["moved_deg"][t, s], max_fill)
        out.append(new)
    return out


def summary(accel, fps: Optional[float] = None) -> Dict[str, float]:
    """Host numbers of an ``accel`` array in metres per frame^2 (a device tensor: one copy): ``n`` defined values and their
    ``mean``, ``median``, ``p95`` and ``max`` in mm/frame^2 (NaN without one); with ``fps`` also ``mean_m_s2`` ... in m/s^2."""
    a = np.asarray(accel.cpu() if hasattr(accel, "cpu") else accel, np.float64).reshape(-1)
    a = a[np.isfinite(a)]
    stats = {"mean": np.mean, "median": np.median, "p95": lambda v: np.percentile(v, 95), "max": np.max}
    out: Dict[str, float] = {"n": int(a.size)}
    for k, fn in stats.items():
        v = float(fn(a)) if a.size else float("nan")
        out[k] = v * 1e3
        if fps is not None:
            out[k + "_m_s2"] = v * float(fps) ** 2
    return out
