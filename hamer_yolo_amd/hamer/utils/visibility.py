"""What the camera sees of each hand (csrc/visibility.hip; the rules are stated in include/hamer_hip.h, "Visibility", and
DESIGN.md section 10.6): a code per joint and vertex (``point_visibility``), pixel counts and boxes per hand
(``mesh_coverage``), both in one go from meshes and joints (``hand_visibility``), and the shares that follow (``summary``).

Everything is judged against the z-buffer and label map of ``render.render_views`` and, when given, a sensor depth map and a
label mask.  Device tensors in, device tensors out, no synchronisation; there is no CPU fallback.

The three default tolerances -- 3 mm for vertices, 15 mm for joints, 10 mm against the sensor -- are choices, not
measurements.  A vertex lies on the rendered surface, so its tolerance only has to absorb the surface's slope across a pixel;
a joint lies UNDER the skin, several millimetres behind the surface that hides it from no one, so it needs the larger one.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Sequence

import numpy as np
import torch

from ... import lib as L
from .depth_eval import _labels_on, _workspace

CODES = ("VISIBLE", "BEHIND", "OUTSIDE", "SELF", "OTHER", "SCENE", "OFF_MASK")
VISIBLE, BEHIND, OUTSIDE, SELF, OTHER, SCENE, OFF_MASK = range(7)
PIXEL_COUNT_NAMES = ("amodal", "modal", "behind_other", "clear", "scene", "unmeasured", "off_mask", "uncovered_in_map")
VERTEX_TOL_M, JOINT_TOL_M, SCENE_TOL_M = 0.003, 0.015, 0.01      # choices, not measurements (module docstring)

_ws: Dict[tuple, torch.Tensor] = {}        # (device index, stream) -> hm_mesh_coverage workspace, grown on demand


def release_workspaces() -> None:
    """Drop the cached coverage workspaces."""
    _ws.clear()


def _upload(a: np.ndarray, dev) -> torch.Tensor:
    """A small host table on the device through pinned memory: the copy is enqueued, the host does not wait for the stream."""
    if a.size == 0:
        return torch.empty(a.shape, dtype=torch.from_numpy(a).dtype, device=dev)
    return torch.from_numpy(np.ascontiguousarray(a)).pin_memory().to(dev, non_blocking=True)


def _labels(who: str, labels, dev, n: int) -> Optional[torch.Tensor]:
    """``depth_eval._labels_on`` without its blocking copy: a sequence is checked on the host and uploaded through pinned memory."""
    if labels is None or torch.is_tensor(labels):
        return _labels_on(who, labels, dev, n)
    a = np.asarray(labels, np.int64).reshape(-1)
    if len(a) != n:
        raise ValueError(f"{who}: labels has {len(a)} entries, expected {n}")
    if ((a < -2) | (a > 255)).any():
        raise ValueError(f"{who}: a label must be -2, -1 or 0..255")
    return _upload(a.astype(np.int32), dev)


def _host_K(who: str, K, N: int) -> np.ndarray:
    Kh = np.asarray(K.cpu() if torch.is_tensor(K) else K, dtype=np.float64)
    Kh = np.broadcast_to(Kh, (N, 3, 3)) if Kh.ndim == 2 else Kh
    if tuple(Kh.shape) != (N, 3, 3):
        raise ValueError(f"{who}: K must be (3,3) or ({N},3,3), got {tuple(Kh.shape)}")
    return np.ascontiguousarray(Kh)


def _check_maps(who: str, depth, mesh_id, sensor, mask):
    if not (torch.is_tensor(depth) and torch.is_tensor(mesh_id)):
        raise ValueError(f"{who}: depth and mesh_id must be tensors")
    dev = mesh_id.device
    if not (mesh_id.is_cuda and depth.device == dev):
        raise ValueError(f"{who}: depth and mesh_id must be on one GPU; there is no CPU path")
    if depth.dtype != torch.float32 or mesh_id.dtype != torch.int32:
        raise ValueError(f"{who}: expected float32 depth and int32 mesh_id, got {depth.dtype}, {mesh_id.dtype}")
    shape = tuple(mesh_id.shape)
    if mesh_id.dim() != 3 or 0 in shape or tuple(depth.shape) != shape:
        raise ValueError(f"{who}: depth {tuple(depth.shape)} / mesh_id {shape}: expected two (N, H, W)")
    if not (depth.is_contiguous() and mesh_id.is_contiguous()):
        raise ValueError(f"{who}: depth and mesh_id must be contiguous")
    if sensor is not None and not (torch.is_tensor(sensor) and sensor.device == dev and sensor.dtype in (torch.uint16, torch.int16)
                                   and tuple(sensor.shape) == shape and sensor.is_contiguous()):
        raise ValueError(f"{who}: sensor must be a contiguous uint16 tensor of shape {shape} on {dev}")
    if mask is not None and not (torch.is_tensor(mask) and mask.device == dev and mask.dtype == torch.uint8
                                 and tuple(mask.shape) == shape and mask.is_contiguous()):
        raise ValueError(f"{who}: mask must be a contiguous uint8 tensor of shape {shape} on {dev}")
    return dev, shape


def _sensor_scalars(who: str, unit, raw_range, scene_tol_m):
    raw_lo, raw_hi = int(raw_range[0]), int(raw_range[1])
    if not (np.isfinite(unit) and unit > 0 and np.isfinite(scene_tol_m) and scene_tol_m > 0):
        raise ValueError(f"{who}: unit and scene_tol_m must be finite and > 0")
    if raw_lo > raw_hi:
        raise ValueError(f"{who}: raw_range must be (lo, hi) with lo <= hi")
    return float(unit), raw_lo, raw_hi, float(scene_tol_m)


def pack_groups(groups: Sequence[dict]) -> np.ndarray:
    """The hm_vis_group table of ``groups`` as host bytes: dicts with ``view``, ``mesh``, ``p0``, ``np``, ``tol_m`` and an
    optional ``label`` (-2: no mask test, the default; -1: mask != 0; 0..255: mask == label)."""
    table = (L.VisGroup * max(len(groups), 1))()
    for i, g in enumerate(groups):
        t = table[i]
        t.tol_m, t.view, t.mesh, t.p0, t.np = float(g["tol_m"]), int(g["view"]), int(g["mesh"]), int(g["p0"]), int(g["np"])
        t.label, t.reserved = int(g.get("label", -2)), 0
    return np.frombuffer(bytes(table), np.uint8)[:len(groups) * C.sizeof(L.VisGroup)].copy()


def point_visibility(depth: torch.Tensor, mesh_id: torch.Tensor, K, points: torch.Tensor, groups, *, window: int = 1,
                     znear: float = 0.05, sensor: Optional[torch.Tensor] = None, unit: float = 0.001, raw_range=(1, 65535),
                     scene_tol_m: float = SCENE_TOL_M, mask: Optional[torch.Tensor] = None, codes: Optional[torch.Tensor] = None):
    """One hm_point_visibility call.  ``depth`` (N, H, W) float32 and ``mesh_id`` (N, H, W) int32 as ``render_views`` returns
    them; ``K`` (3,3) or (N,3,3) on the host; ``points`` (P, 3) camera-frame, on the maps' GPU (converted to float64);
    ``groups``: a sequence of dicts (``pack_groups``) or a uint8 device tensor holding the packed table.  ``window``: 0, 1 or 2
    pixels around the projected point.  ``sensor`` (N, H, W) uint16 with ``unit``, ``raw_range`` and ``scene_tol_m``, and
    ``mask`` (N, H, W) uint8 (tested with each group's ``label``) are optional.  Returns ``(codes (P,) uint8, counts (G, 8)
    int32)`` on the device: ``CODES[c]`` names code c; counts[g][c] is the number of group g's points with code c, counts[g][7]
    its size.  Points in no group keep what ``codes`` held (a new tensor holds 255 there).  Enqueued on the current stream
    without synchronising."""
    who = "point_visibility"
    dev, (N, H, W) = _check_maps(who, depth, mesh_id, sensor, mask)
    if int(window) not in (0, 1, 2):
        raise ValueError(f"{who}: window must be 0, 1 or 2, got {window}")
    if not (np.isfinite(znear) and znear > 0):
        raise ValueError(f"{who}: znear must be finite and > 0")
    unit, raw_lo, raw_hi, scene_tol_m = _sensor_scalars(who, unit, raw_range, scene_tol_m)
    Kh = _host_K(who, K, N)
    if not (torch.is_tensor(points) and points.device == dev and points.dim() == 2 and points.shape[1] == 3):
        raise ValueError(f"{who}: points must be a (P, 3) tensor on {dev}")
    pts = points.to(torch.float64).contiguous()
    P = int(pts.shape[0])
    if torch.is_tensor(groups):
        if not (groups.device == dev and groups.dtype == torch.uint8 and groups.dim() == 1 and groups.is_contiguous()
                and groups.numel() % C.sizeof(L.VisGroup) == 0):
            raise ValueError(f"{who}: a groups tensor must be the packed table, contiguous uint8 on {dev}")
        gd = groups
    else:
        gd = _upload(pack_groups(groups), dev)
    G = gd.numel() // C.sizeof(L.VisGroup)
    if codes is None:
        codes = torch.full((P,), 255, dtype=torch.uint8, device=dev)
    elif not (codes.device == dev and codes.dtype == torch.uint8 and tuple(codes.shape) == (P,) and codes.is_contiguous()):
        raise ValueError(f"{who}: codes must be a contiguous uint8 tensor of shape ({P},) on {dev}")
    counts = torch.empty(G, 8, dtype=torch.int32, device=dev)
    if G == 0:
        return codes, counts
    lib = L.load()
    with torch.cuda.device(dev):
        L.check(lib.hm_point_visibility(L.ptr(depth), L.ptr(mesh_id), N, H, W, Kh.ctypes.data_as(C.POINTER(C.c_double)), float(znear),
                                        L.ptr(pts) if P else None, P, L.ptr(gd), G, int(window), L.ptr(sensor), unit, raw_lo, raw_hi,
                                        scene_tol_m, L.ptr(mask), L.ptr(codes) if P else None, L.ptr(counts), L.current_stream()),
                "hm_point_visibility")
    return codes, counts


def mesh_coverage(H: int, W: int, K, meshes: Sequence[dict], depth: torch.Tensor, mesh_id: torch.Tensor, *,
                  znear: float = 0.05, sensor: Optional[torch.Tensor] = None, unit: float = 0.001, raw_range=(1, 65535),
                  scene_tol_m: float = SCENE_TOL_M, mask: Optional[torch.Tensor] = None, labels=None):
    """One hm_mesh_coverage call: ``meshes`` in ``render_views``'s format (the SAME list, in the same order, that produced
    ``depth`` and ``mesh_id``), ``K`` (3,3) or (N,3,3).  ``labels``: per mesh -2, -1 or 0..255, tested against ``mask``; both
    or neither.  Returns ``(counts (n_meshes, 8) int64 -- PIXEL_COUNT_NAMES --, boxes (n_meshes, 8) int32: x1, y1, x2, y2 of the
    amodal, then of the modal pixels, -1 where there are none)`` on the device.  Enqueued on the current stream without
    synchronising; the workspace is cached per device and stream (``release_workspaces``)."""
    from ...render import _pack_meshes
    who = "mesh_coverage"
    dev, (N, h, w) = _check_maps(who, depth, mesh_id, sensor, mask)
    if (h, w) != (int(H), int(W)):
        raise ValueError(f"{who}: the maps are {h} x {w}, not {H} x {W}")
    if (mask is None) != (labels is None):
        raise ValueError(f"{who}: mask and labels are given both or neither")
    if not (np.isfinite(znear) and znear > 0):
        raise ValueError(f"{who}: znear must be finite and > 0")
    unit, raw_lo, raw_hi, scene_tol_m = _sensor_scalars(who, unit, raw_range, scene_tol_m)
    Kh = _host_K(who, K, N)
    n = len(meshes)
    lab = _labels(who, labels, dev, n)
    table, vd, fd, v0, f0 = _pack_meshes(meshes, dev, N)
    counts = torch.empty(n, 8, dtype=torch.int64, device=dev)
    boxes = torch.empty(n, 8, dtype=torch.int32, device=dev)
    if n == 0:
        return counts, boxes
    lib = L.load()
    with torch.cuda.device(dev):
        stream = L.current_stream()
        ws = _workspace(_ws, dev, stream, int(lib.hm_mesh_coverage_workspace_bytes(N, h, w, v0, n, f0)))
        L.check(lib.hm_mesh_coverage(N, h, w, Kh.ctypes.data_as(C.POINTER(C.c_double)), L.ptr(vd) if v0 else None, v0,
                                     L.ptr(fd) if f0 else None, f0, table, n, float(znear), L.ptr(depth), L.ptr(mesh_id),
                                     L.ptr(sensor), unit, raw_lo, raw_hi, scene_tol_m, L.ptr(mask), L.ptr(lab), L.ptr(counts),
                                     L.ptr(boxes), L.ptr(ws), ws.numel() * 8, stream), "hm_mesh_coverage")
    return counts, boxes


def hand_visibility(H: int, W: int, K, meshes: Sequence[dict], joints, *, vertex_tol_m: float = VERTEX_TOL_M,
                    joint_tol_m: float = JOINT_TOL_M, window: int = 1, znear: float = 0.05, sensor: Optional[torch.Tensor] = None,
                    unit: float = 0.001, raw_range=(1, 65535), scene_tol_m: float = SCENE_TOL_M,
                    mask: Optional[torch.Tensor] = None, labels=None, views: Optional[int] = None) -> Dict[str, torch.Tensor]:
    """Visibility of n hands: ``meshes`` in ``render_views``'s format (hand i is mesh i, drawn into view ``frame``) and
    ``joints`` (n, J, 3) camera-frame on the meshes' GPU.  One ``render_views`` call (depth and mesh_id), one
    hm_point_visibility call with two groups per hand -- its vertices at ``vertex_tol_m``, its joints at ``joint_tol_m`` --
    and one hm_mesh_coverage call.  ``labels``: per hand, with ``mask``.  ``vertex_tol_m``, ``joint_tol_m`` and
    ``scene_tol_m`` default to choices, not measurements; joints lie under the skin and need the larger one.
    Returns device tensors, without synchronising (``render_views`` reads a mesh's face range back once unless the mesh says
    ``faces_checked``): ``vertex_codes`` (total vertices,) uint8 in mesh order with
    ``vertex_start`` (n + 1,) host offsets, ``joint_codes`` (n, J) uint8, ``counts_points`` (n, 2, 8) int32 (vertices,
    joints), ``counts_pixels`` (n, 8) int64, ``boxes`` (n, 8) int32, and the render's ``depth`` and ``mesh_id``."""
    from ...render import render_views
    n = len(meshes)
    if n == 0:
        raise ValueError("hand_visibility: no hands")
    if (mask is None) != (labels is None):
        raise ValueError("hand_visibility: mask and labels are given both or neither")
    r = render_views(H, W, K, meshes, outputs=("depth", "mesh_id"), znear=znear, views=views,
                     device=sensor.device if sensor is not None else mask.device if mask is not None else None)
    depth, mesh_id = r["depth"], r["mesh_id"]
    dev = depth.device
    j = torch.as_tensor(joints).to(dev, torch.float64)
    if j.dim() != 3 or j.shape[0] != n or j.shape[2] != 3:
        raise ValueError(f"hand_visibility: joints must be ({n}, J, 3), got {tuple(j.shape)}")
    J = int(j.shape[1])
    verts = [torch.as_tensor(m["vertices"]).to(dev, torch.float64).reshape(-1, 3) for m in meshes]
    start = np.concatenate([[0], np.cumsum([int(v.shape[0]) for v in verts])]).astype(np.int64)
    V = int(start[-1])
    lab = [-2] * n if labels is None else [int(x) for x in (labels.cpu().tolist() if torch.is_tensor(labels) else labels)]
    groups = []
    for i, m in enumerate(meshes):
        groups.append({"view": m["frame"], "mesh": i, "p0": int(start[i]), "np": int(start[i + 1] - start[i]),
                       "tol_m": vertex_tol_m, "label": lab[i]})
        groups.append({"view": m["frame"], "mesh": i, "p0": V + i * J, "np": J, "tol_m": joint_tol_m, "label": lab[i]})
    points = torch.cat(verts + [j.reshape(-1, 3)])
    kw = dict(znear=znear, sensor=sensor, unit=unit, raw_range=raw_range, scene_tol_m=scene_tol_m, mask=mask)
    codes, counts = point_visibility(depth, mesh_id, K, points, groups, window=window, **kw)
    checked = [dict(m, faces_checked=True) for m in meshes]                # render_views has looked at the faces
    cpix, boxes = mesh_coverage(H, W, K, checked, depth, mesh_id, labels=None if labels is None else lab, **kw)
    return {"vertex_codes": codes[:V], "vertex_start": start, "joint_codes": codes[V:].reshape(n, J),
            "counts_points": counts.reshape(n, 2, 8), "counts_pixels": cpix, "boxes": boxes, "depth": depth, "mesh_id": mesh_id}


def summary(counts_points, counts_pixels) -> Dict[str, np.ndarray]:
    """Host numpy, float64.  ``counts_points`` (n, 8) (or (n, 2, 8): the VERTEX rows are taken) and ``counts_pixels`` (n, 8),
    device tensors (one copy each) or arrays.  Per hand: ``visible_share`` = clear / amodal, ``occluded_by_hand`` =
    behind_other / amodal, ``occluded_by_scene`` = scene / amodal (all NaN at amodal == 0) and ``in_frame`` = 1 - (BEHIND +
    OUTSIDE vertices) / vertices (NaN without vertices)."""
    cp = np.asarray(counts_points.cpu() if torch.is_tensor(counts_points) else counts_points).astype(np.int64)
    cp = cp[:, 0, :] if cp.ndim == 3 else cp.reshape(-1, 8)
    cx = np.asarray(counts_pixels.cpu() if torch.is_tensor(counts_pixels) else counts_pixels).astype(np.int64).reshape(-1, 8)
    if len(cp) != len(cx):
        raise ValueError(f"summary: {len(cp)} point rows for {len(cx)} pixel rows")
    amodal = cx[:, 0].astype(np.float64)
    nv = cp[:, 7].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        share = lambda k: np.where(amodal > 0, cx[:, k].astype(np.float64) / amodal, np.nan)      # noqa: E731
        in_frame = np.where(nv > 0, 1.0 - (cp[:, BEHIND] + cp[:, OUTSIDE]).astype(np.float64) / nv, np.nan)
        return {"visible_share": share(3), "occluded_by_hand": share(2), "occluded_by_scene": share(4), "in_frame": in_frame}
