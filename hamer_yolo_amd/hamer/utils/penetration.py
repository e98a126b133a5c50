"""Do two hand meshes pass through each other (csrc/penetration.hip; the rule is stated in include/hamer_hip.h, "Penetration",
and DESIGN.md section 10.7): per ordered pair of meshes the signed distance of every vertex of the first to the surface of the
second (``mesh_penetration``), both directions of every two-hand frame (``hand_penetration``), the numbers that follow
(``summary``), and a translation that takes the hands apart (``resolve_penetration``).

Device tensors in, device tensors out, no synchronisation; there is no CPU fallback.  The inside test counts ray crossings and
therefore needs a closed surface: ``close_boundaries`` gives the faces that close a mesh's holes (the MANO wrist), and the
drivers append them for this feature only.  The default contact tolerance, 2 mm, is a choice, not a measurement.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from ... import lib as L
from .depth_eval import _workspace

CODES = ("FAR", "NEAR", "INSIDE", "INVALID")
FAR, NEAR, INSIDE, INVALID = range(4)
STATUSES = ("OK", "DISJOINT", "TOO_LARGE")
SUM_NAMES = ("tested", "near", "inside", "invalid", "status", "max_depth_bits", "sum_depth", "push_x", "push_y", "push_z")
CONTACT_TOL_M = 0.002                      # a choice, not a measurement (module docstring)
GAIN = 1.125                               # resolve_penetration: step = GAIN * the larger maximum depth
QUANTA = 65536.0                           # the rule's fixed point: quanta per metre

_ws: Dict[tuple, torch.Tensor] = {}        # (device index, stream) -> hm_mesh_penetration workspace, grown on demand


def release_workspaces() -> None:
    """Drop the cached workspaces."""
    _ws.clear()


def close_boundaries(faces, n_verts: int) -> np.ndarray:
    """The faces that close the holes of a mesh, (K, 3) int32, without adding a vertex: the boundary edges (used by exactly
    one face) are chained into loops and each loop is fanned from its lowest-index vertex, running against its faces' direction
    so that the fan faces outward with them.  A closed mesh gets (0, 3).  Host numpy."""
    f = np.asarray(faces.cpu() if torch.is_tensor(faces) else faces, np.int64).reshape(-1, 3)
    if len(f) and (f.min() < 0 or f.max() >= n_verts):
        raise ValueError("close_boundaries: a corner index outside the vertices")
    directed: Dict[tuple, int] = {}
    for a, b in np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]).tolist():
        directed[(a, b)] = directed.get((a, b), 0) + 1
    nxt: Dict[int, int] = {}
    for (a, b), k in directed.items():
        if k + directed.get((b, a), 0) == 1:
            if b in nxt:
                raise ValueError("close_boundaries: two boundary loops touch at a vertex")
            nxt[b] = a
    extra: List[tuple] = []
    while nxt:
        start = min(nxt)
        loop, v = [start], nxt.pop(start)
        while v != start:
            loop.append(v)
            if v not in nxt:
                raise ValueError("close_boundaries: a boundary chain does not close")
            v = nxt.pop(v)
        extra += [(loop[0], loop[i], loop[i + 1]) for i in range(1, len(loop) - 1)]
    return np.asarray(extra, np.int32).reshape(-1, 3)


def closed_faces(faces, n_verts: int) -> np.ndarray:
    """``faces`` with ``close_boundaries``'s faces appended: (F + K, 3) int32 on the host."""
    f = np.asarray(faces.cpu() if torch.is_tensor(faces) else faces, np.int32).reshape(-1, 3)
    return np.concatenate([f, close_boundaries(f, n_verts)])


def pack_queries(pairs: Sequence, n_meshes: int):
    """The hm_pen_query table of ``pairs`` ((a, b) mesh rows), checked on the host."""
    table = (L.PenQuery * max(len(pairs), 1))()
    for q, (a, b) in enumerate(pairs):
        if not (0 <= int(a) < n_meshes and 0 <= int(b) < n_meshes):
            raise ValueError(f"mesh_penetration: pair {q} = ({a}, {b}) names a mesh outside the {n_meshes} given")
        table[q].a, table[q].b = int(a), int(b)
    return table


def _device_of(meshes: Sequence[dict]) -> torch.device:
    for m in meshes:
        if torch.is_tensor(m["vertices"]) and m["vertices"].is_cuda:
            return m["vertices"].device
    raise ValueError("mesh_penetration: the vertices must be tensors on a GPU; there is no CPU path")


def _pack(meshes: Sequence[dict], dev):
    from ...render import _pack_meshes
    # the kernel skips a face with a corner outside its mesh, so the faces need no look from the host (faces_checked)
    return _pack_meshes([dict(m, frame=int(m.get("frame", 0)), faces_checked=True) for m in meshes], dev, 2 ** 31 - 1)


def _run(table, vd, fd, n_verts: int, n_faces: int, n_meshes: int, queries, n_queries: int, rows: int, contact_tol_m: float):
    dev = vd.device
    code = torch.empty(rows, dtype=torch.uint8, device=dev)
    sd = torch.empty(rows, dtype=torch.float32, device=dev)
    near = torch.empty(rows, dtype=torch.int32, device=dev)
    sums = torch.empty(n_queries, 10, dtype=torch.int64, device=dev)
    if n_queries == 0:
        return code, sd, near, sums
    lib = L.load()
    with torch.cuda.device(dev):
        stream = L.current_stream()
        ws = _workspace(_ws, dev, stream, int(lib.hm_mesh_penetration_workspace_bytes(n_verts, n_meshes, n_queries)))
        L.check(lib.hm_mesh_penetration(L.ptr(vd) if n_verts else None, n_verts, L.ptr(fd) if n_faces else None, n_faces, table, n_meshes,
                                        queries, n_queries, float(contact_tol_m), L.ptr(code) if rows else None,
                                        L.ptr(sd) if rows else None, L.ptr(near) if rows else None, rows, L.ptr(sums), L.ptr(ws),
                                        ws.numel() * 8, stream), "hm_mesh_penetration")
    return code, sd, near, sums


def _check_tol(contact_tol_m) -> float:
    if not (np.isfinite(contact_tol_m) and 0.0 <= contact_tol_m <= 1.0):
        raise ValueError(f"mesh_penetration: contact_tol_m must lie in 0 .. 1 m, got {contact_tol_m}")
    return float(contact_tol_m)


def _row_start(meshes: Sequence[dict], pairs: Sequence) -> np.ndarray:
    nv = [int(np.prod(tuple(m["vertices"].shape)) // 3) for m in meshes]
    return np.concatenate([[0], np.cumsum([nv[int(a)] for a, _ in pairs])]).astype(np.int64)


def mesh_penetration(meshes: Sequence[dict], pairs: Sequence, contact_tol_m: float = CONTACT_TOL_M,
                     stream: Optional[torch.cuda.Stream] = None) -> Dict[str, object]:
    """One hm_mesh_penetration call.  ``meshes``: the dicts ``render.render_views`` takes (``vertices`` (nv, 3) camera-frame on
    a GPU, ``faces`` (nf, 3) with corners relative to the mesh; ``frame`` is not used).  ``pairs``: ordered (a, b) mesh rows:
    the vertices of a against the surface of b, which should be closed (``close_boundaries``).  Returns device tensors:
    ``code`` (rows,) uint8 (``CODES``), ``signed_distance`` (rows,) float32 (negative inside, +inf FAR, NaN INVALID),
    ``nearest_face`` (rows,) int32 (the face's index in b, or -1) and ``sums`` (len(pairs), 10) int64 (``SUM_NAMES``), with
    ``row_start`` (len(pairs) + 1,) host offsets: pair q owns rows row_start[q] .. row_start[q + 1] - 1, one per vertex of a.
    Enqueued on ``stream`` (default: the current one) without synchronising; the workspace is cached per device and stream
    (``release_workspaces``)."""
    tol = _check_tol(contact_tol_m)
    n = len(meshes)
    queries = pack_queries(pairs, n)
    start = _row_start(meshes, pairs)
    if n == 0:
        raise ValueError("mesh_penetration: no meshes")
    dev = _device_of(meshes)
    with torch.cuda.stream(stream) if stream is not None else torch.cuda.device(dev):
        table, vd, fd, v0, f0 = _pack(meshes, dev)
        code, sd, near, sums = _run(table, vd, fd, v0, f0, n, queries, len(pairs), int(start[-1]), tol)
    return {"code": code, "signed_distance": sd, "nearest_face": near, "sums": sums, "row_start": start}


def hand_pairs(meshes: Sequence[dict]) -> List[tuple]:
    """The unordered pairs (i, j), i < j, of the frames that hold exactly two meshes (``frame`` of the mesh dicts)."""
    by_frame: Dict[int, List[int]] = {}
    for i, m in enumerate(meshes):
        by_frame.setdefault(int(m["frame"]), []).append(i)
    return [(v[0], v[1]) for _, v in sorted(by_frame.items()) if len(v) == 2]


def hand_penetration(meshes: Sequence[dict], contact_tol_m: float = CONTACT_TOL_M, stream=None) -> Dict[str, object]:
    """Both directions of every two-hand frame in one call: for each frame with exactly two meshes (i, j) the queries (i, j)
    and (j, i), in this order.  Returns ``mesh_penetration``'s result with ``pairs`` (the ordered pairs submitted) and
    ``hands`` (the unordered ones); frames with one mesh, or more than two, take no part."""
    hands = hand_pairs(meshes)
    pairs = [p for i, j in hands for p in ((i, j), (j, i))]
    if not pairs:
        dev = _device_of(meshes)
        e = lambda t: torch.empty(0, dtype=t, device=dev)                # noqa: E731
        r = {"code": e(torch.uint8), "signed_distance": e(torch.float32), "nearest_face": e(torch.int32),
             "sums": torch.empty(0, 10, dtype=torch.int64, device=dev), "row_start": np.zeros(1, np.int64)}
    else:
        r = mesh_penetration(meshes, pairs, contact_tol_m, stream)
    r["pairs"], r["hands"] = pairs, hands
    return r


def summary(sums) -> Dict[str, np.ndarray]:
    """Host numpy of ``sums`` (Q, 10) (a device tensor: one copy, or an array).  Per query: ``max_depth_m`` and
    ``mean_depth_m`` over the inside vertices (0.0 without one), ``inside``, ``contact`` (NEAR), ``tested`` and ``invalid``
    vertex counts and ``status`` (``STATUSES``)."""
    s = np.ascontiguousarray(np.asarray(sums.cpu() if torch.is_tensor(sums) else sums).astype(np.int64).reshape(-1, 10))
    inside = s[:, 2]
    mean = np.where(inside > 0, s[:, 6].astype(np.float64) / 4294967296.0 / np.maximum(inside, 1), 0.0)
    return {"max_depth_m": s[:, 5].copy().view(np.float64), "mean_depth_m": mean, "inside": inside.copy(), "contact": s[:, 1].copy(),
            "tested": s[:, 0].copy(), "invalid": s[:, 3].copy(), "status": s[:, 4].copy()}


def resolve_penetration(meshes: Sequence[dict], pairs: Sequence, rounds: int = 8, gain: float = GAIN,
                        contact_tol_m: float = CONTACT_TOL_M) -> Dict[str, object]:
    """Translate the two meshes of every pair apart until no vertex of one lies inside the other: ``rounds`` times measure
    (both directions of every pair, one kernel call) then move, all on the device without host synchronisation.  ``pairs``:
    unordered (i, j) mesh rows; a mesh should appear in one pair only.  Per round and pair the direction is the normalised
    D = push(i, j) - push(j, i) (the push vector of a query is the sum over its inside vertices of closest surface point minus
    vertex), the length ``gain`` times the larger of the two maximum depths; i moves by +half of it, j by -half, rounded to
    the rule's quantum (2^-16 m).  The step is zero once no vertex is inside (or when D vanishes).  Only translations: a hand's
    record takes its shift as ``cam_t + shift``.  Returns ``shift`` (n, 3) float64 metres and ``shift_quanta`` (n, 3) int64
    per mesh, the measurement after the last move (``code``, ``signed_distance``, ``nearest_face``, ``sums``, ``row_start``,
    ``pairs`` as ``hand_penetration`` orders them) and ``resolved`` (len(pairs),) bool: no vertex inside afterwards."""
    tol = _check_tol(contact_tol_m)
    if int(rounds) < 0 or not (np.isfinite(gain) and gain > 0):
        raise ValueError("resolve_penetration: rounds must be >= 0 and gain finite and > 0")
    n = len(meshes)
    dev = _device_of(meshes)
    ordered = [p for i, j in pairs for p in ((int(i), int(j)), (int(j), int(i)))]
    queries = pack_queries(ordered, n)
    start = _row_start(meshes, ordered)
    P = len(pairs)
    with torch.cuda.device(dev):
        table, base, fd, v0, f0 = _pack(meshes, dev)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).pin_memory().to(dev, non_blocking=True) if a.size else \
            torch.empty(a.shape, dtype=torch.int64, device=dev)          # noqa: E731
        owner = up(np.repeat(np.arange(n, dtype=np.int64), [table[i].nv for i in range(n)]))
        pi, pj = up(np.array([i for i, _ in pairs], np.int64)), up(np.array([j for _, j in pairs], np.int64))
        tq = torch.zeros(n, 3, dtype=torch.int64, device=dev)
        measure = lambda: _run(table, base + tq.to(torch.float64)[owner] * (1.0 / QUANTA), fd, v0, f0, n, queries, 2 * P,  # noqa: E731
                               int(start[-1]), tol)
        for _ in range(int(rounds) if P else 0):
            sums = measure()[3]
            s1, s2 = sums[0::2], sums[1::2]
            D = (s1[:, 7:10] - s2[:, 7:10]).to(torch.float64)
            norm = torch.sqrt((D[:, 0] * D[:, 0] + D[:, 1] * D[:, 1]) + D[:, 2] * D[:, 2])
            depth = torch.maximum(s1[:, 5].contiguous().view(torch.float64), s2[:, 5].contiguous().view(torch.float64))
            length = gain * depth
            go = ((s1[:, 2] + s2[:, 2]) > 0) & (norm > 0)
            half = torch.where(go[:, None], torch.round(D / norm[:, None] * (length * 0.5)[:, None] * QUANTA), 0.0).to(torch.int64)
            tq.index_add_(0, pi, half)
            tq.index_add_(0, pj, -half)
        code, sd, near, sums = measure()
    resolved = (sums[0::2, 2] + sums[1::2, 2]) == 0
    return {"shift": tq.to(torch.float64) * (1.0 / QUANTA), "shift_quanta": tq, "code": code, "signed_distance": sd, "nearest_face": near,
            "sums": sums, "row_start": start, "pairs": ordered, "resolved": resolved}
