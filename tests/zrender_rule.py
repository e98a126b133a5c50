"""numpy restatement of the z-buffered renderer's rule (include/hamer_hip.h, hm_mesh_render), the
oracle of tests/test_zrender_host.py and tests/test_gpu_zrender.py.  Vectorised over faces like render_rule: every face's
clipped pixel box is expanded into (face, pixel) pairs, the edge functions run on all pairs in int64, the fp64 depth on the
covered pairs, and the smallest key per pixel wins.  numpy never contracts a product and a sum, and its fp64 division and
square root are IEEE, so every expression below is the rule's, in the rule's order."""
import numpy as np

from render_rule import _edge

LIMIT = 65536.0
CHUNK_PAIRS = 1 << 22
NO_KEY = np.iinfo(np.uint64).max
BASE_RGB = (1.0, 1.0, 0.9)


def project(vertices, K, znear):
    """(V,3) fp64 camera-frame vertices -> 24.8 fixed-point (V,2) int64, 1/z (V,), and a validity mask."""
    v = np.asarray(vertices, np.float64).reshape(-1, 3)
    K = np.asarray(K, np.float64)
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    with np.errstate(all="ignore"):
        u = ((K[0, 0] * x + K[0, 1] * y) + K[0, 2] * z) / z
        w = ((K[1, 0] * x + K[1, 1] * y) + K[1, 2] * z) / z
        ok = (z >= znear) & (np.abs(u) < LIMIT) & (np.abs(w) < LIMIT)
        r = 1.0 / z
    fx = np.zeros((len(v), 2), np.int64)
    fx[ok, 0] = np.rint(256.0 * u[ok]).astype(np.int64)
    fx[ok, 1] = np.rint(256.0 * w[ok]).astype(np.int64)
    return fx, r, ok


def vertex_normals(vertices, faces):
    """(V,3) fp64: per vertex the sum, from zero and in ascending face row, of (p1-p0) x (p2-p0) over the faces with three
    valid corner indices that name it (once per face)."""
    v = np.asarray(vertices, np.float64).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    f = f[((f >= 0) & (f < len(v))).all(1)]
    n = np.zeros_like(v)
    if len(f) == 0:
        return n
    p0, p1, p2 = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    a, c = p1 - p0, p2 - p0
    term = np.stack([a[:, 1] * c[:, 2] - a[:, 2] * c[:, 1], a[:, 2] * c[:, 0] - a[:, 0] * c[:, 2],
                     a[:, 0] * c[:, 1] - a[:, 1] * c[:, 0]], 1)
    # corner columns one after another would break the row order, so scatter face by face position: a stable sort of the
    # (vertex, row) incidences, then np.add.at, which applies repeated indices in the order given
    rows = np.arange(len(f))
    inc_v = np.concatenate([f[:, 0], f[:, 1], f[:, 2]])
    inc_r = np.concatenate([rows, rows, rows])
    keep = np.ones(len(inc_v), bool)                                    # a face naming a vertex twice counts once
    keep[len(f):2 * len(f)] &= f[:, 1] != f[:, 0]
    keep[2 * len(f):] &= (f[:, 2] != f[:, 0]) & (f[:, 2] != f[:, 1])
    inc_v, inc_r = inc_v[keep], inc_r[keep]
    order = np.lexsort((inc_r, inc_v))
    np.add.at(n, inc_v[order], term[inc_r[order]])
    return n


def face_table(vertices, faces, K, znear):
    """Per face of one mesh, in the rule's corner order (1 and 2 swapped where the area was negative): corners (F,3,2) int64,
    r (F,3), corner vertex indices (F,3), twice the area (F,) int64 > 0 where valid, valid (F,)."""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    nv = len(vertices)
    if nv == 0 or len(faces) == 0:
        z = np.zeros
        return z((len(faces), 3, 2), np.int64), z((len(faces), 3)), z((len(faces), 3), np.int64), z(len(faces), np.int64), z(len(faces), bool)
    inside = ((faces >= 0) & (faces < nv)).all(1)
    fc = np.where(inside[:, None], faces, 0)
    fx, r, ok = project(vertices, K, znear)
    corners, rr = fx[fc], r[fc]
    valid = inside & ok[fc].all(1)
    X, Y = corners[:, :, 0], corners[:, :, 1]
    area = _edge(X[:, 0], Y[:, 0], X[:, 1], Y[:, 1], X[:, 2], Y[:, 2])
    swap = area < 0
    perm = np.where(swap[:, None], np.array([0, 2, 1]), np.array([0, 1, 2]))
    idx = np.arange(len(faces))[:, None]
    corners, rr, fc = corners[idx, perm], rr[idx, perm], fc[idx, perm]
    area = np.abs(area)
    valid &= area != 0
    return corners, rr, fc, area, valid


def _owns(ax, ay, bx, by):
    dy, dx = by - ay, bx - ax
    return (dy < 0) | ((dy == 0) & (dx > 0))


def edge_values(corners, sx, sy):
    """E_0, E_1, E_2 (edges 1->2, 2->0, 0->1) of faces `corners` (n,3,2) at the samples (sx, sy) (n,), and the covered mask."""
    X, Y = corners[:, :, 0], corners[:, :, 1]
    E, hit = [], np.ones(len(corners), bool)
    for a, b in ((1, 2), (2, 0), (0, 1)):
        e = _edge(X[:, a], Y[:, a], X[:, b], Y[:, b], sx, sy)
        hit &= (e > 0) | ((e == 0) & _owns(X[:, a], Y[:, a], X[:, b], Y[:, b]))
        E.append(e)
    return E, hit


def cover_pairs(corners, H, W):
    """(face index, pixel index y*W+x, E_0, E_1, E_2) of every covered in-view pixel centre."""
    if len(corners) == 0:
        z = np.zeros(0, np.int64)
        return z, z, [z, z, z]
    x, y = corners[:, :, 0], corners[:, :, 1]
    bx0, bx1 = np.maximum((x.min(1) + 127) >> 8, 0), np.minimum((x.max(1) - 128) >> 8, W - 1)
    by0, by1 = np.maximum((y.min(1) + 127) >> 8, 0), np.minimum((y.max(1) - 128) >> 8, H - 1)
    bw, bh = np.maximum(bx1 - bx0 + 1, 0), np.maximum(by1 - by0 + 1, 0)
    n = bw * bh
    fi = np.repeat(np.arange(len(corners)), n)
    start = np.repeat(np.cumsum(n) - n, n)
    local = np.arange(int(n.sum()), dtype=np.int64) - start
    px = bx0[fi] + local % np.maximum(bw[fi], 1)
    py = by0[fi] + local // np.maximum(bw[fi], 1)
    E, hit = edge_values(corners[fi], 256 * px + 128, 256 * py + 128)
    return fi[hit], (py * W + px)[hit], [e[hit] for e in E]


def pair_depth(E, area, r):
    """d (float32) of covered pairs: E three (n,) int64, area (n,) int64, r (n,3)."""
    A = area.astype(np.float64)
    l0, l1, l2 = E[0].astype(np.float64) / A, E[1].astype(np.float64) / A, E[2].astype(np.float64) / A
    q = (l0 * r[:, 0] + l1 * r[:, 1]) + l2 * r[:, 2]
    with np.errstate(over="ignore"):
        return (1.0 / q).astype(np.float32)


def _pixel_box_area(cv, H, W):
    x, y = cv[:, :, 0], cv[:, :, 1]
    bw = np.minimum((x.max(1) - 128) >> 8, W - 1) - np.maximum((x.min(1) + 127) >> 8, 0) + 1
    bh = np.minimum((y.max(1) - 128) >> 8, H - 1) - np.maximum((y.min(1) + 127) >> 8, 0) + 1
    return np.maximum(bw, 0) * np.maximum(bh, 0)


def render(N, H, W, K, meshes, base_rgb=BASE_RGB, bg_rgba=(0, 0, 0, 0), znear=0.05, frames=None):
    """meshes: list of dicts {frame (the view), vertices (V,3), faces (F,3) relative to the mesh, face_id0 (global id of its
    first face)}; a mesh's label is its position in the list.  Returns a dict: key (N,H,W) uint64, rgba (N,H,W,4) uint8,
    depth (N,H,W) float32, mesh_id (N,H,W) int32, face (N,H,W) int64 (global id, -1 = none) and, with `frames`
    (N,H,W,3) uint8 BGR, out."""
    K = np.asarray(K, np.float64)
    K = np.broadcast_to(K, (N, 3, 3)) if K.ndim == 2 else K
    best = np.full((N, H * W), NO_KEY, np.uint64)
    tables = []
    for mi, m in enumerate(meshes):
        v = np.asarray(m["vertices"], np.float64).reshape(-1, 3)
        corners, rr, fc, area, valid = face_table(v, m["faces"], K[m["frame"]], znear)
        f0 = int(m.get("face_id0", 0))
        tables.append((f0, len(corners), mi, corners, rr, fc, area, vertex_normals(v, m["faces"])))
        sel = np.nonzero(valid)[0]
        cv = corners[sel]
        boxes = _pixel_box_area(cv, H, W)
        bounds = np.searchsorted(np.cumsum(boxes), np.arange(1, int(boxes.sum()) // CHUNK_PAIRS + 1) * CHUNK_PAIRS)
        for lo, hi in zip(np.r_[0, bounds], np.r_[bounds, len(cv)]):          # at most ~CHUNK_PAIRS (face, pixel) pairs at once
            if hi <= lo:
                continue
            fi, pix, E = cover_pairs(cv[lo:hi], H, W)
            rows = sel[lo:hi][fi]
            d = pair_depth(E, area[rows], rr[rows])
            key = (d.view(np.uint32).astype(np.uint64) << np.uint64(32)) | (rows.astype(np.uint64) + np.uint64(f0))
            np.minimum.at(best[m["frame"]], pix, key)
    base = np.asarray(base_rgb, np.float64)
    rgba = np.empty((N, H * W, 4), np.uint8)
    rgba[:] = np.asarray(bg_rgba, np.uint8)
    depth = np.zeros((N, H * W), np.float32)
    mesh_id = np.full((N, H * W), -1, np.int32)
    face = np.full((N, H * W), -1, np.int64)
    for n in range(N):
        hit = np.nonzero(best[n] != NO_KEY)[0]
        if len(hit) == 0:
            continue
        fid = (best[n][hit] & np.uint64(0xFFFFFFFF)).astype(np.int64)
        face[n, hit] = fid
        depth[n, hit] = (best[n][hit] >> np.uint64(32)).astype(np.uint32).view(np.float32)
        for f0, nf, mi, corners, rr, fc, area, normals in tables:
            s = (fid >= f0) & (fid < f0 + nf)
            if not s.any():
                continue
            rows, pix = fid[s] - f0, hit[s]
            mesh_id[n, pix] = mi
            E, _ = edge_values(corners[rows], 256 * (pix % W) + 128, 256 * (pix // W) + 128)
            A = area[rows].astype(np.float64)
            a = [E[i].astype(np.float64) / A * rr[rows, i] for i in range(3)]
            nn = normals[fc[rows]]                                           # (n, 3 corners, 3 components)
            mv = [(a[0] * nn[:, 0, c] + a[1] * nn[:, 1, c]) + a[2] * nn[:, 2, c] for c in range(3)]
            with np.errstate(all="ignore"):
                ln = np.sqrt((mv[0] * mv[0] + mv[1] * mv[1]) + mv[2] * mv[2])
                t = np.where(ln > 0, np.abs(mv[2]) / ln, 0.0)
                inten = 0.3 + 0.7 * t
                col = np.stack([255.0 * base[c] * inten for c in range(3)], 1)
                col = np.clip(np.where(np.isnan(col), 0.0, np.rint(col)), 0, 255).astype(np.uint8)
            rgba[n, pix, :3] = col
            rgba[n, pix, 3] = 255
    out = {"key": best.reshape(N, H, W), "rgba": rgba.reshape(N, H, W, 4), "depth": depth.reshape(N, H, W),
           "mesh_id": mesh_id.reshape(N, H, W), "face": face.reshape(N, H, W)}
    if frames is not None:
        o = np.asarray(frames, np.uint8).copy()
        cov = out["face"] >= 0
        o[cov] = out["rgba"][..., 2::-1][cov]
        out["out"] = o
    return out
