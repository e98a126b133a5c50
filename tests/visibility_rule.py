"""numpy restatement of the two visibility rules (include/hamer_hip.h, "Visibility"), the oracle of
tests/test_visibility_host.py and tests/test_gpu_visibility.py.  The point rule is a plain loop over points, every fp64
expression in the rule's order (numpy never contracts a product and a sum).  Coverage comes from zrender_rule's face table and
covered (face, pixel) pairs, de-duplicated per mesh and pixel."""
import numpy as np

import zrender_rule as ZR

VISIBLE, BEHIND, OUTSIDE, SELF, OTHER, SCENE, OFF_MASK = range(7)
AMODAL, MODAL, BEHIND_OTHER, CLEAR, PX_SCENE, UNMEASURED, PX_OFF_MASK, UNCOVERED = range(8)


def mask_passes(value, label):
    if label == -1:
        return value != 0
    return 0 <= label <= 255 and value == label


def point_code(pt, g, depth, mesh_id, K, znear, window, sensor=None, unit=0.001, raw_range=(1, 65535), scene_tol_m=0.01,
               mask=None):
    """The code of one point of group g (a dict: tol_m, view, mesh, label)."""
    N, H, W = mesh_id.shape
    x, y, z = (np.float64(c) for c in pt)
    if not z >= np.float64(znear):
        return BEHIND
    view = int(g["view"])
    if not 0 <= view < N:
        return OUTSIDE
    k = np.asarray(K, np.float64)
    k = k if k.ndim == 2 else k[view]
    with np.errstate(all="ignore"):
        u = ((k[0, 0] * x + k[0, 1] * y) + k[0, 2] * z) / z
        v = ((k[1, 0] * x + k[1, 1] * y) + k[1, 2] * z) / z
    if not (abs(u) < 65536.0 and abs(v) < 65536.0):
        return OUTSIDE
    px, py = int(np.rint(256.0 * u)) >> 8, int(np.rint(256.0 * v)) >> 8
    if not (0 <= px < W and 0 <= py < H):
        return OUTSIDE
    win = [(px + dx, py + dy) for dy in range(-window, window + 1) for dx in range(-window, window + 1)
           if 0 <= px + dx < W and 0 <= py + dy < H]
    zt = z - np.float64(g["tol_m"])
    ok = False
    for xx, yy in win:
        if mesh_id[view, yy, xx] >= 0:
            ok = ok or np.float64(depth[view, yy, xx]) >= zt
        else:
            ok = ok or (xx == px and yy == py)
    if not ok:
        return SELF if mesh_id[view, py, px] == int(g["mesh"]) else OTHER
    if sensor is not None:
        zs = z - np.float64(scene_tol_m)
        any_valid = clear = False
        for xx, yy in win:
            raw = int(sensor[view, yy, xx])
            if raw == 0 or raw < raw_range[0] or raw > raw_range[1]:
                continue
            any_valid = True
            clear = clear or np.float64(raw) * np.float64(unit) >= zs
        if any_valid and not clear:
            return SCENE
    label = int(g.get("label", -2))
    if mask is not None and label != -2 and not mask_passes(int(mask[view, py, px]), label):
        return OFF_MASK
    return VISIBLE


def point_visibility(depth, mesh_id, K, points, groups, window=1, znear=0.05, codes=None, **kw):
    """(codes (P,) uint8, counts (G, 8) int32).  Points in no group keep what `codes` held (255 in a new array)."""
    points = np.asarray(points, np.float64).reshape(-1, 3)
    P = len(points)
    codes = np.full(P, 255, np.uint8) if codes is None else np.array(codes, np.uint8)
    counts = np.zeros((len(groups), 8), np.int32)
    for gi, g in enumerate(groups):
        p0, n = int(g["p0"]), int(g["np"])
        if n <= 0 or p0 < 0 or p0 + n > P:
            continue
        counts[gi, 7] = n
        for i in range(p0, p0 + n):
            c = point_code(points[i], g, depth, mesh_id, K, znear, window, **kw)
            codes[i] = c
            counts[gi, c] += 1
    return codes, counts


def covered_by(mesh, K, H, W, znear=0.05):
    """(H*W,) bool: the pixels some non-skipped face of the mesh covers."""
    corners, rr, fc, area, valid = ZR.face_table(np.asarray(mesh["vertices"], np.float64).reshape(-1, 3), mesh["faces"], K, znear)
    cov = np.zeros(H * W, bool)
    fi, pix, E = ZR.cover_pairs(corners[valid], H, W)
    cov[pix] = True
    return cov


def classify(cov, m, depth, mesh_id, sensor=None, unit=0.001, raw_range=(1, 65535), scene_tol_m=0.01, mask=None, label=-2):
    """counts (8,) int64 and boxes (8,) int32 of mesh row m from its coverage `cov` (H, W) and its view's maps (H, W)."""
    H, W = cov.shape
    cls = np.zeros((8, H, W), bool)
    cls[AMODAL] = cov
    cls[MODAL] = cov & (mesh_id == m)
    cls[BEHIND_OTHER] = cov & (mesh_id >= 0) & (mesh_id != m)
    cls[UNCOVERED] = cov & (mesh_id < 0)
    scene = np.zeros((H, W), bool)
    if sensor is not None:
        raw = sensor.astype(np.int64)
        valid = (raw != 0) & (raw >= raw_range[0]) & (raw <= raw_range[1])
        scene = valid & (raw.astype(np.float64) * np.float64(unit) < depth.astype(np.float64) - np.float64(scene_tol_m))
        cls[UNMEASURED] = cls[MODAL] & ~valid
    off = np.zeros((H, W), bool)
    if mask is not None and label is not None and label != -2:
        passes = (mask != 0) if label == -1 else ((mask == label) if 0 <= label <= 255 else np.zeros((H, W), bool))
        off = ~passes
    cls[PX_SCENE] = cls[MODAL] & scene
    cls[PX_OFF_MASK] = cls[MODAL] & ~scene & off
    cls[CLEAR] = cls[MODAL] & ~scene & ~off
    boxes = np.full(8, -1, np.int32)
    for k in (0, 1):
        ys, xs = np.nonzero(cls[k])
        if len(ys):
            boxes[4 * k:4 * k + 4] = xs.min(), ys.min(), xs.max(), ys.max()
    return cls.reshape(8, -1).sum(1).astype(np.int64), boxes


def mesh_coverage(H, W, K, meshes, depth, mesh_id, znear=0.05, sensor=None, mask=None, labels=None, **kw):
    """(counts (n, 8) int64, boxes (n, 8) int32) of meshes in zrender_rule.render's format."""
    N = mesh_id.shape[0]
    K = np.asarray(K, np.float64)
    K = np.broadcast_to(K, (N, 3, 3)) if K.ndim == 2 else K
    counts, boxes = np.zeros((len(meshes), 8), np.int64), np.full((len(meshes), 8), -1, np.int32)
    for m, mesh in enumerate(meshes):
        n = int(mesh["frame"])
        cov = covered_by(mesh, K[n], H, W, znear).reshape(H, W)
        counts[m], boxes[m] = classify(cov, m, depth[n], mesh_id[n], None if sensor is None else sensor[n],
                                       mask=None if mask is None else mask[n],
                                       label=-2 if (labels is None or mask is None) else int(labels[m]), **kw)
    return counts, boxes


def summary(counts_points, counts_pixels):
    cp, cx = np.asarray(counts_points, np.int64).reshape(-1, 8), np.asarray(counts_pixels, np.int64).reshape(-1, 8)
    out = {k: np.full(len(cx), np.nan) for k in ("visible_share", "occluded_by_hand", "occluded_by_scene", "in_frame")}
    for i in range(len(cx)):
        if cx[i, 0] > 0:
            out["visible_share"][i] = float(cx[i, CLEAR]) / float(cx[i, 0])
            out["occluded_by_hand"][i] = float(cx[i, BEHIND_OTHER]) / float(cx[i, 0])
            out["occluded_by_scene"][i] = float(cx[i, PX_SCENE]) / float(cx[i, 0])
        if cp[i, 7] > 0:
            out["in_frame"][i] = 1.0 - float(cp[i, BEHIND] + cp[i, OUTSIDE]) / float(cp[i, 7])
    return out
