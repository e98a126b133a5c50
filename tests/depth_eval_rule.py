"""numpy restatement of the depth-residual rule (include/hamer_hip.h, "Depth residuals"), the oracle of
tests/test_depth_eval_host.py and tests/test_gpu_depth_eval.py: the per-pixel rule, the statistics, the host summary and the
refine loop.  numpy never contracts a product and a sum and its fp64 division is IEEE, so every expression below is the
rule's, in the rule's order."""
import numpy as np

COUNT_NAMES = ("covered", "off_mask", "no_measurement", "below", "above", "in_range", "reserved6", "reserved7")


def residuals(pred_depth, pred_id, sensor, mesh_query, Q, unit=0.001, bin_m=0.0005, bins=4096, raw_range=(1, 65535), mask=None,
              labels=None):
    """(hist (Q, bins) int64, counts (Q, 8) int64) of (N, H, W) arrays, vectorised over the pixels."""
    d = np.asarray(pred_depth, np.float32).reshape(-1)
    pid = np.asarray(pred_id, np.int64).reshape(-1)
    raw = np.asarray(sensor, np.uint16).reshape(-1).astype(np.int64)
    mq = np.asarray(mesh_query, np.int64).reshape(-1)
    hist, counts = np.zeros((Q, bins), np.int64), np.zeros((Q, 8), np.int64)
    ok = (pid >= 0) & (pid < len(mq))
    q = np.full(len(pid), -1, np.int64)
    q[ok] = mq[pid[ok]]
    ok &= (q >= 0) & (q < Q)
    np.add.at(counts[:, 0], q[ok], 1)
    if mask is not None and labels is not None:
        m = np.asarray(mask, np.uint8).reshape(-1).astype(np.int64)
        lab = np.full(len(pid), -2, np.int64)
        lab[ok] = np.asarray(labels, np.int64)[q[ok]]
        fail = ok & (lab != -2) & ~np.where(lab == -1, m != 0, m == lab)
        np.add.at(counts[:, 1], q[fail], 1)
        ok &= ~fail
    none = ok & ((raw == 0) | (raw < raw_range[0]) | (raw > raw_range[1]))
    np.add.at(counts[:, 2], q[none], 1)
    ok &= ~none
    r = raw[ok].astype(np.float64) * np.float64(unit) - d[ok].astype(np.float64)
    with np.errstate(invalid="ignore"):
        t = np.floor(r / np.float64(bin_m))
        above = ~(t < 2.0 ** 40)
        below = t < -2.0 ** 40
    k = np.where(above | below, 0, t).astype(np.int64) + bins // 2
    below |= ~above & (k < 0)
    above |= ~below & (k >= bins)
    qq = q[ok]
    inside = ~(below | above)
    np.add.at(counts[:, 3], qq[below], 1)
    np.add.at(counts[:, 4], qq[above], 1)
    np.add.at(counts[:, 5], qq[inside], 1)
    np.add.at(hist, (qq[inside], k[inside]), 1)
    return hist, counts


def residuals_loop(pred_depth, pred_id, sensor, mesh_query, Q, unit=0.001, bin_m=0.0005, bins=4096, raw_range=(1, 65535), mask=None,
                   labels=None):
    """The same, pixel by pixel, in the words of the header."""
    d, pid, raw = np.asarray(pred_depth, np.float32).reshape(-1), np.asarray(pred_id).reshape(-1), np.asarray(sensor, np.uint16).reshape(-1)
    m = None if mask is None or labels is None else np.asarray(mask, np.uint8).reshape(-1)
    hist, counts = np.zeros((Q, bins), np.int64), np.zeros((Q, 8), np.int64)
    for p in range(len(pid)):
        i = int(pid[p])
        if not 0 <= i < len(mesh_query):
            continue
        q = int(mesh_query[i])
        if not 0 <= q < Q:
            continue
        counts[q, 0] += 1
        if m is not None and labels[q] != -2 and not (m[p] != 0 if labels[q] == -1 else m[p] == labels[q]):
            counts[q, 1] += 1
            continue
        v = int(raw[p])
        if v == 0 or v < raw_range[0] or v > raw_range[1]:
            counts[q, 2] += 1
            continue
        r = np.float64(v) * np.float64(unit) - np.float64(d[p])
        t = np.floor(r / np.float64(bin_m))
        if not t < 2.0 ** 40:
            counts[q, 4] += 1
            continue
        if t < -2.0 ** 40:
            counts[q, 3] += 1
            continue
        k = int(t) + bins // 2
        if k < 0:
            counts[q, 3] += 1
        elif k >= bins:
            counts[q, 4] += 1
        else:
            hist[q, k] += 1
            counts[q, 5] += 1
    return hist, counts


def centre(k, bins, bin_m):
    return (np.float64(k - bins // 2) + 0.5) * np.float64(bin_m)


def stats(hist, counts, bin_m):
    """(Q, 4) float64: lower median, mean, mean absolute, rms."""
    Q, bins = hist.shape
    out = np.full((Q, 4), np.nan)
    for q in range(Q):
        below, above, inside = (int(counts[q, i]) for i in (3, 4, 5))
        n = below + inside + above
        m = (n + 1) // 2
        s1 = s2 = s3 = np.float64(0.0)
        cum, found = below, False
        for k in np.nonzero(hist[q])[0]:
            c, w = centre(int(k), bins, bin_m), np.float64(hist[q, k])
            s1 = s1 + w * c
            s2 = s2 + w * np.abs(c)
            s3 = s3 + w * (c * c)
            cum += int(hist[q, k])
            if n > 0 and below < m <= below + inside and not found and cum >= m:
                out[q, 0], found = c, True
        if inside:
            out[q, 1], out[q, 2], out[q, 3] = s1 / np.float64(inside), s2 / np.float64(inside), np.sqrt(s3 / np.float64(inside))
    return out


def summary(hist, counts, bin_m, thresholds_m=(0.005, 0.010, 0.020)):
    """What hamer.utils.depth_eval.summary_from_hist states, query by query."""
    Q, bins = hist.shape
    st = stats(hist, counts, bin_m)
    cs = np.array([centre(k, bins, bin_m) for k in range(bins)])
    valid = counts[:, 3] + counts[:, 4] + counts[:, 5]
    out = {"median": st[:, 0], "mean_abs": st[:, 2], "valid": valid, "covered": counts[:, 0],
           "inliers": np.full((Q, len(thresholds_m)), np.nan), "measured": np.full(Q, np.nan), "occluded": np.full(Q, np.nan)}
    for q in range(Q):
        if valid[q]:
            out["inliers"][q] = [hist[q][np.abs(cs) <= t].sum() / valid[q] for t in thresholds_m]
            out["occluded"][q] = counts[q, 3] / valid[q]
        if counts[q, 0]:
            out["measured"][q] = valid[q] / counts[q, 0]
    return out


def refine_step(cam_t, median, counts, min_pixels=200, min_fraction=0.25, znear=0.05):
    """One update of the refine loop: (cam_t' (B, 3) of cam_t's dtype, ok (B,) bool)."""
    cam_t = np.asarray(cam_t)
    valid = counts[:, 3] + counts[:, 4] + counts[:, 5]
    tz = cam_t[:, 2].astype(np.float64)
    with np.errstate(all="ignore"):
        ok = np.isfinite(median) & (valid >= min_pixels) & (valid.astype(np.float64) / counts[:, 0].astype(np.float64) >= min_fraction) \
            & (tz + median > znear)
        moved = (cam_t.astype(np.float64) * ((tz + median) / tz)[:, None]).astype(cam_t.dtype)
    return np.where(ok[:, None], moved, cam_t), ok


def refine(render, vertices, cam_t, sensor, unit, iterations=2, min_pixels=200, min_fraction=0.25, znear=0.05, bin_m=0.0005,
           bins=4096, raw_range=(1, 65535), mask=None, labels=None):
    """The refine loop: ``render(placed vertices (B, V, 3)) -> (depth, mesh_id)`` with mesh j the hand j.  Returns (cam_t, the
    last median, the last valid counts, updated, the cam_t after each iteration)."""
    cur = np.asarray(cam_t).copy()
    B = len(cur)
    updated, trail = np.zeros(B, bool), []
    median, valid = np.full(B, np.nan), np.zeros(B, np.int64)
    for _ in range(iterations):
        depth, mid = render(vertices + cur[:, None, :].astype(vertices.dtype))
        hist, counts = residuals(depth, mid, sensor, np.arange(B), B, unit, bin_m, bins, raw_range, mask, labels)
        median, valid = stats(hist, counts, bin_m)[:, 0], counts[:, 3] + counts[:, 4] + counts[:, 5]
        cur, ok = refine_step(cur, median, counts, min_pixels, min_fraction, znear)
        updated |= ok
        trail.append(cur.copy())
    return cur, median, valid, updated, trail


def ellipsoid(semi=(0.05, 0.08, 0.02), n_lat=24, n_lon=48):
    """A closed triangle mesh of the ellipsoid with the given semi-axes about the origin: (vertices (V, 3) float64, faces (F, 3))."""
    lat = np.linspace(0.0, np.pi, n_lat + 1)[1:-1]
    lon = np.linspace(0.0, 2 * np.pi, n_lon, endpoint=False)
    ring = np.stack([np.outer(np.sin(lat), np.cos(lon)), np.outer(np.sin(lat), np.sin(lon)), np.outer(np.cos(lat), np.ones_like(lon))], -1)
    v = np.concatenate([[[0.0, 0.0, 1.0]], ring.reshape(-1, 3), [[0.0, 0.0, -1.0]]]) * np.asarray(semi, np.float64)
    f = []
    for j in range(n_lon):
        f.append((0, 1 + j, 1 + (j + 1) % n_lon))
        last = 1 + (n_lat - 2) * n_lon
        f.append((len(v) - 1, last + (j + 1) % n_lon, last + j))
    for i in range(n_lat - 2):
        a, b = 1 + i * n_lon, 1 + (i + 1) * n_lon
        for j in range(n_lon):
            j1 = (j + 1) % n_lon
            f += [(a + j, b + j, b + j1), (a + j, b + j1, a + j1)]
    return v, np.asarray(f, np.int32)


def sensor_from_depth(depth, unit, wall_m=None):
    """A raw uint16 sensor image of a float depth render: rint(depth / unit), the uncovered pixels at ``wall_m`` (None: 0)."""
    d = np.asarray(depth, np.float64)
    if wall_m is not None:
        d = np.where(d > 0, d, wall_m)
    return np.clip(np.rint(d / unit), 0, 65535).astype(np.uint16)


def contraction_maps(seed, N, H, W, n_meshes):
    """(depth, pred_id, sensor) on which a fused multiply-subtract shows with unit = 0.001 and bin_m = 0.0005: every depth is a
    multiple of 1/8 m, exact in fp32 and a whole number of millimetres, and every raw value a whole number of millimetres from
    it, so each residual sits on a bin edge up to the rounding of raw * unit -- which a fused operation does not perform."""
    rng = np.random.default_rng(seed)
    a = rng.integers(1, 9, (N, H, W))
    depth = (a * 0.125).astype(np.float32)
    sensor = (125 * a + rng.integers(-20, 21, (N, H, W))).astype(np.uint16)
    pid = rng.integers(-1, n_meshes, (N, H, W)).astype(np.int32)
    return np.where(pid >= 0, depth, np.float32(0)), pid, sensor


def fused_bins(depth, sensor, unit=0.001, bin_m=0.0005, bins=4096):
    """The bin of every pixel had r been computed as fma(raw, unit, -depth): one rounding of the exact value."""
    from fractions import Fraction
    d, raw = np.asarray(depth, np.float32).reshape(-1), np.asarray(sensor).reshape(-1)
    r = np.array([float(Fraction(int(v)) * Fraction(float(unit)) - Fraction(float(x))) for v, x in zip(raw, d)])
    return np.floor(r / np.float64(bin_m)).astype(np.int64) + bins // 2
