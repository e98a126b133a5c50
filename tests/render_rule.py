"""numpy restatement of the mesh overlay rule (include/hamer_hip.h, hm_mesh_overlay), the oracle of
tests/test_render_host.py and tests/test_gpu_render.py.  Vectorised over faces: every face's clipped bounding box is expanded
into (face, pixel) pairs, the closed-triangle test runs on all pairs in int64, and the smallest key per pixel wins."""
import numpy as np

LIMIT = float(1 << 24)
CHUNK_PAIRS = 1 << 22


def project(vertices, K):
    """(V,3) fp64 camera-frame vertices -> integer pixels (V,2) int64 and a per-vertex validity mask (z > 0, |u|, |v| < 2^24).
    No contraction, in the rule's order; z == 0 becomes 1e-5 first."""
    v = np.asarray(vertices, np.float64)
    K = np.asarray(K, np.float64)
    x, y, z0 = v[:, 0], v[:, 1], v[:, 2]
    z = np.where(z0 == 0.0, 1e-5, z0)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        w = (K[2, 0] * x + K[2, 1] * y) + K[2, 2] * z
        u = ((K[0, 0] * x + K[0, 1] * y) + K[0, 2] * z) / w
        vv = ((K[1, 0] * x + K[1, 1] * y) + K[1, 2] * z) / w
        ok = (z0 > 0) & (np.abs(u) < LIMIT) & (np.abs(vv) < LIMIT)
    px = np.zeros((len(v), 2), np.int64)
    px[ok, 0] = u[ok].astype(np.int32)
    px[ok, 1] = vv[ok].astype(np.int32)
    return px, ok


def shade_colors(vertices, faces):
    """HM_STYLE_SHADED colour (B, G, R) uint8 per face."""
    v = np.asarray(vertices, np.float64)
    p0, p1, p2 = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
    a, c = p1 - p0, p2 - p0
    nx = a[:, 1] * c[:, 2] - a[:, 2] * c[:, 1]
    ny = a[:, 2] * c[:, 0] - a[:, 0] * c[:, 2]
    nz = a[:, 0] * c[:, 1] - a[:, 1] * c[:, 0]
    ln = np.sqrt((nx * nx + ny * ny) + nz * nz)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(ln > 0, np.abs(nz) / ln, 0.0)
    inten = 0.3 + 0.7 * t
    out = np.stack([255.0 * 0.9 * inten, 255.0 * 1.0 * inten, 255.0 * 1.0 * inten], 1)
    return np.clip(np.rint(out), 0, 255).astype(np.uint8)


def face_table(vertices, faces, K, face_id0=0):
    """Per face of one mesh: corners (F,3,2) int64, valid (F,), key (F,) uint64."""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    nv = len(vertices)
    inside = ((faces >= 0) & (faces < nv)).all(1)
    fc = np.where(inside[:, None], faces, 0)
    px, ok = project(vertices, K) if nv else (np.zeros((0, 2), np.int64), np.zeros(0, bool))
    if nv == 0:
        return np.zeros((0, 3, 2), np.int64), np.zeros(0, bool), np.zeros(0, np.uint64)
    corners = px[fc]
    valid = inside & ok[fc].all(1)
    z = np.asarray(vertices, np.float64)[:, 2][fc]
    depth = (((z[:, 0] + z[:, 1]) + z[:, 2]) / 3.0).astype(np.float32)
    key = (depth.view(np.uint32).astype(np.uint64) << np.uint64(32)) | (np.arange(len(faces), dtype=np.uint64) + np.uint64(face_id0))
    return corners, valid, key


def _edge(ax, ay, bx, by, px, py):
    return (bx - ax) * (py - ay) - (by - ay) * (px - ax)


def cover_pairs(corners, H, W):
    """(face index, pixel index y*W+x) of every covered in-frame pixel, for faces given by their integer corners."""
    if len(corners) == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    x, y = corners[:, :, 0], corners[:, :, 1]
    bx0, bx1 = np.maximum(x.min(1), 0), np.minimum(x.max(1), W - 1)
    by0, by1 = np.maximum(y.min(1), 0), np.minimum(y.max(1), H - 1)
    bw, bh = np.maximum(bx1 - bx0 + 1, 0), np.maximum(by1 - by0 + 1, 0)
    n = bw * bh
    fi = np.repeat(np.arange(len(corners)), n)
    start = np.repeat(np.cumsum(n) - n, n)
    local = np.arange(int(n.sum()), dtype=np.int64) - start
    px = bx0[fi] + local % bw[fi]
    py = by0[fi] + local // bw[fi]
    X, Y = x[fi], y[fi]
    e0 = _edge(X[:, 0], Y[:, 0], X[:, 1], Y[:, 1], px, py)
    e1 = _edge(X[:, 1], Y[:, 1], X[:, 2], Y[:, 2], px, py)
    e2 = _edge(X[:, 2], Y[:, 2], X[:, 0], Y[:, 0], px, py)
    area = _edge(X[:, 0], Y[:, 0], X[:, 1], Y[:, 1], X[:, 2], Y[:, 2])
    tri = ((e0 >= 0) & (e1 >= 0) & (e2 >= 0)) | ((e0 <= 0) & (e1 <= 0) & (e2 <= 0))

    def seg(e, a, b):
        return ((e == 0) & (px >= np.minimum(X[:, a], X[:, b])) & (px <= np.maximum(X[:, a], X[:, b]))
                & (py >= np.minimum(Y[:, a], Y[:, b])) & (py <= np.maximum(Y[:, a], Y[:, b])))

    deg = seg(e0, 0, 1) | seg(e1, 1, 2) | seg(e2, 2, 0)
    hit = np.where(area != 0, tri, deg)
    return fi[hit], (py * W + px)[hit]


def overlay(frames, K, meshes, style="flat", alpha=0.6):
    """frames (N,H,W,3) uint8; K (N,3,3) or (3,3); meshes: list of dicts {frame, vertices (V,3), faces (F,3) relative to the
    mesh, face_id0 (global id of its first face), color (B, G, R)}.  Returns the overlaid frames (a new array)."""
    frames = np.asarray(frames, np.uint8)
    N, H, W, _ = frames.shape
    K = np.asarray(K, np.float64)
    K = np.broadcast_to(K, (N, 3, 3)) if K.ndim == 2 else K
    out = frames.copy()
    best = np.full((N, H * W), np.iinfo(np.uint64).max, np.uint64)
    colour = {}
    for m in meshes:
        f = m["frame"]
        corners, valid, key = face_table(m["vertices"], m["faces"], K[f], m.get("face_id0", 0))
        if style == "shaded":
            cols = shade_colors(m["vertices"], np.where(valid[:, None], np.asarray(m["faces"], np.int64), 0)) if len(key) else np.zeros((0, 3), np.uint8)
        else:
            cols = np.tile(np.asarray(m.get("color", (0, 255, 0)), np.uint8), (len(key), 1))
        for k, c in zip(key[valid].tolist(), cols[valid]):
            colour[k & 0xFFFFFFFF] = c
        cv, kv = corners[valid], key[valid]
        area = (np.clip(cv[:, :, 0].max(1), -1, W) - np.clip(cv[:, :, 0].min(1), -1, W) + 1) * \
               (np.clip(cv[:, :, 1].max(1), -1, H) - np.clip(cv[:, :, 1].min(1), -1, H) + 1)
        bounds = np.searchsorted(np.cumsum(area), np.arange(1, int(area.sum()) // CHUNK_PAIRS + 1) * CHUNK_PAIRS)
        for lo, hi in zip(np.r_[0, bounds], np.r_[bounds, len(cv)]):          # at most ~CHUNK_PAIRS (face, pixel) pairs at once
            if hi > lo:
                fi, pix = cover_pairs(cv[lo:hi], H, W)
                np.minimum.at(best[f], pix, kv[lo:hi][fi])
    a, b = np.float32(alpha), np.float32(1.0 - alpha)
    for n in range(N):
        hit = np.nonzero(best[n] != np.iinfo(np.uint64).max)[0]
        if len(hit) == 0:
            continue
        ids = (best[n][hit] & np.uint64(0xFFFFFFFF)).astype(np.int64)
        uniq, inv = np.unique(ids, return_inverse=True)
        c = np.stack([colour[int(i)] for i in uniq])[inv]
        img = out[n].reshape(-1, 3)
        if style == "shaded":
            img[hit] = c
        else:
            i = img[hit].astype(np.float32)
            img[hit] = np.clip(np.rint(a * c.astype(np.float32) + b * i), 0, 255).astype(np.uint8)
    return out
