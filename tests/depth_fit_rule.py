"""numpy restatement of the depth-fit rule (include/hamer_hip.h, "Depth fit"), the oracle of
tests/test_depth_fit_host.py and tests/test_gpu_depth_fit.py: the per-pixel rule with its integer sums, the damped Cholesky
solve, the rigid loop and the folding of a fit into a record.  numpy never contracts a product and a sum and its fp64 division
and square root are IEEE, so every expression below is the rule's, in the rule's order."""
import numpy as np

COUNT_NAMES = ("covered", "off_mask", "no_measurement", "gated", "no_normal", "rejected", "used", "reserved7")
SCALE = np.float64(2.0 ** 30)
PAIRS = [(i, j) for i in range(6) for j in range(i, 6)]                               # the 21 pairs, i <= j, row by row


def cameras_of(K, N):
    """(N, 4) float64 fx, fy, cx, cy of K (3, 3) or (N, 3, 3)."""
    K = np.asarray(K, np.float64)
    K = np.broadcast_to(K, (N, 3, 3)) if K.ndim == 2 else K
    return np.ascontiguousarray(np.stack([K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2]], 1))


def _terms(J, rho, l2):
    """(n, 28) int64 of J (n, 6), rho (n,), l2 (n,)."""
    out = np.zeros((len(rho), 28), np.int64)
    for k, (i, j) in enumerate(PAIRS):
        out[:, k] = np.rint((J[:, i] * J[:, j]) / l2 * SCALE).astype(np.int64)
    for i in range(6):
        out[:, 21 + i] = np.rint((J[:, i] * rho) / l2 * SCALE).astype(np.int64)
    out[:, 27] = np.rint((rho * rho) / l2 * SCALE).astype(np.int64)
    return out


def fit(pred_depth, pred_id, sensor, mesh_query, Q, cameras, pivot, unit=0.001, gate_m=0.03, edge_m=0.005, reach_m=0.5,
        raw_range=(1, 65535), mask=None, labels=None, parts=False):
    """(sums (Q, 28) int64, counts (Q, 8) int64) of (N, H, W) arrays, vectorised over the pixels.  ``parts=True`` also returns
    (pixel indices, queries, J, rho, l2) of the used pixels."""
    N, H, W = np.asarray(pred_id).shape
    d32 = np.asarray(pred_depth, np.float32).reshape(-1)
    pid = np.asarray(pred_id, np.int64).reshape(-1)
    raw = np.asarray(sensor, np.uint16).reshape(-1).astype(np.int64)
    mq = np.asarray(mesh_query, np.int64).reshape(-1)
    cam, pv = np.asarray(cameras, np.float64).reshape(N, 4), np.asarray(pivot, np.float64).reshape(-1, 3)
    sums, counts = np.zeros((Q, 28), np.int64), np.zeros((Q, 8), np.int64)
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
    d = d32.astype(np.float64)
    with np.errstate(all="ignore"):
        rz = raw.astype(np.float64) * np.float64(unit) - d
        gated = ok & ~(np.abs(rz) <= np.float64(gate_m))
    np.add.at(counts[:, 3], q[gated], 1)
    ok &= ~gated
    e = np.arange(len(pid))
    rem = e % (H * W)
    n, v, u = e // (H * W), rem // W, rem % W
    inner = (u >= 1) & (u + 1 < W) & (v >= 1) & (v + 1 < H)
    idx = np.nonzero(ok & inner)[0]
    good = np.zeros(len(pid), bool)
    with np.errstate(all="ignore"):
        g = np.ones(len(idx), bool)
        for off in (-1, 1, -W, W):
            g &= (pid[idx + off] == pid[idx]) & (np.abs(d[idx + off] - d[idx]) <= np.float64(edge_m))
    good[idx[g]] = True
    bad = ok & ~good
    np.add.at(counts[:, 4], q[bad], 1)
    ok &= good
    i = np.nonzero(ok)[0]
    qi, di, rzi = q[i], d[i], rz[i]
    fx, fy, cx, cy = (cam[n[i], k] for k in range(4))
    ui, vi = u[i].astype(np.float64), v[i].astype(np.float64)
    dl, dr, du, dd = d[i - 1], d[i + 1], d[i - W], d[i + W]
    with np.errstate(all="ignore"):
        rx, rxl, rxr = (ui - cx) / fx, ((ui - 1.0) - cx) / fx, ((ui + 1.0) - cx) / fx
        ry, ryu, ryd = (vi - cy) / fy, ((vi - 1.0) - cy) / fy, ((vi + 1.0) - cy) / fy
        ax, ay, az = dr * rxr - dl * rxl, dr * ry - dl * ry, dr - dl
        bx, by, bz = dd * rx - du * rx, dd * ryd - du * ryu, dd - du
        nx, ny, nz = ay * bz - az * by, az * bx - ax * bz, ax * by - ay * bx
        l2 = nx * nx + ny * ny + nz * nz
        mx, my, mz = di * rx - pv[qi, 0], di * ry - pv[qi, 1], di - pv[qi, 2]
        rho = (nx * rx + ny * ry + nz) * rzi
        mm = mx * mx + my * my + mz * mz
        rej = ~((l2 > 0.0) & (l2 <= np.finfo(np.float64).max)) | (mm > np.float64(reach_m) * np.float64(reach_m)) | (rho * rho > l2)
        J = np.stack([my * nz - mz * ny, mz * nx - mx * nz, mx * ny - my * nx, nx, ny, nz], 1)
    np.add.at(counts[:, 5], qi[rej], 1)
    use = ~rej
    np.add.at(counts[:, 6], qi[use], 1)
    t = _terms(J[use], rho[use], l2[use])
    np.add.at(sums, qi[use], t)
    if parts:
        return sums, counts, (i[use], qi[use], J[use], rho[use], l2[use])
    return sums, counts


def fit_loop(pred_depth, pred_id, sensor, mesh_query, Q, cameras, pivot, unit=0.001, gate_m=0.03, edge_m=0.005, reach_m=0.5,
             raw_range=(1, 65535), mask=None, labels=None):
    """The same, pixel by pixel, in the words of the header; Python ints for the sums."""
    N, H, W = np.asarray(pred_id).shape
    d32, pid = np.asarray(pred_depth, np.float32).reshape(-1), np.asarray(pred_id).reshape(-1)
    raw = np.asarray(sensor, np.uint16).reshape(-1)
    m = None if mask is None or labels is None else np.asarray(mask, np.uint8).reshape(-1)
    cam, pv = np.asarray(cameras, np.float64).reshape(N, 4), np.asarray(pivot, np.float64).reshape(-1, 3)
    f = np.float64
    unit, gate_m, edge_m, reach_m = f(unit), f(gate_m), f(edge_m), f(reach_m)
    sums = [[0] * 28 for _ in range(Q)]
    counts = np.zeros((Q, 8), np.int64)
    with np.errstate(all="ignore"):
        for e in range(len(pid)):
            i = int(pid[e])
            if not 0 <= i < len(mesh_query):
                continue
            q = int(mesh_query[i])
            if not 0 <= q < Q:
                continue
            counts[q, 0] += 1
            if m is not None and labels[q] != -2 and not (m[e] != 0 if labels[q] == -1 else m[e] == labels[q]):
                counts[q, 1] += 1
                continue
            r = int(raw[e])
            if r == 0 or r < raw_range[0] or r > raw_range[1]:
                counts[q, 2] += 1
                continue
            d = f(d32[e])
            rz = f(r) * unit - d
            if not np.abs(rz) <= gate_m:
                counts[q, 3] += 1
                continue
            n, rem = divmod(e, H * W)
            v, u = divmod(rem, W)
            nb = [e - 1, e + 1, e - W, e + W]
            if u < 1 or u + 1 >= W or v < 1 or v + 1 >= H or any(int(pid[k]) != i for k in nb) \
                    or any(not np.abs(f(d32[k]) - d) <= edge_m for k in nb):
                counts[q, 4] += 1
                continue
            dl, dr, du, dd = (f(d32[k]) for k in nb)
            fx, fy, cx, cy = cam[n]
            rx, rxl, rxr = (f(u) - cx) / fx, (f(u - 1) - cx) / fx, (f(u + 1) - cx) / fx
            ry, ryu, ryd = (f(v) - cy) / fy, (f(v - 1) - cy) / fy, (f(v + 1) - cy) / fy
            a = (dr * rxr - dl * rxl, dr * ry - dl * ry, dr - dl)
            b = (dd * rx - du * rx, dd * ryd - du * ryu, dd - du)
            nx, ny, nz = a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]
            l2 = nx * nx + ny * ny + nz * nz
            mx, my, mz = d * rx - pv[q, 0], d * ry - pv[q, 1], d - pv[q, 2]
            rho = (nx * rx + ny * ry + nz) * rz
            mm = mx * mx + my * my + mz * mz
            if not (l2 > 0.0 and l2 <= np.finfo(np.float64).max) or mm > reach_m * reach_m or rho * rho > l2:
                counts[q, 5] += 1
                continue
            counts[q, 6] += 1
            J = (my * nz - mz * ny, mz * nx - mx * nz, mx * ny - my * nx, nx, ny, nz)
            for k, (a_, b_) in enumerate(PAIRS):
                sums[q][k] += int(np.rint((J[a_] * J[b_]) / l2 * SCALE))
            for k in range(6):
                sums[q][21 + k] += int(np.rint((J[k] * rho) / l2 * SCALE))
            sums[q][27] += int(np.rint((rho * rho) / l2 * SCALE))
    return np.array(sums, np.int64).reshape(Q, 28), counts


def matrix(sums_q, used, damping, lever_m):
    """(M (6, 6), g (6,)) of one query's 28 sums."""
    inv = np.float64(2.0 ** -30)
    M, g = np.zeros((6, 6)), np.zeros(6)
    for k, (i, j) in enumerate(PAIRS):
        M[i, j] = M[j, i] = np.float64(int(sums_q[k])) * inv
    for i in range(6):
        g[i] = np.float64(int(sums_q[21 + i])) * inv
    du = np.float64(damping) * np.float64(int(used))
    lever2 = np.float64(lever_m) * np.float64(lever_m)
    for i in range(3):
        M[i, i] = M[i, i] + du * lever2
    for i in range(3, 6):
        M[i, i] = M[i, i] + du
    return M, g


def cholesky_solve(M, g):
    """(x, every pivot > 0) by the header's order: column by column, inner sums from k = 0 upwards."""
    L = np.zeros((6, 6))
    ok = True
    with np.errstate(all="ignore"):
        for j in range(6):
            s = M[j, j]
            for k in range(j):
                s = s - L[j, k] * L[j, k]
            if not s > 0.0:
                ok = False
            L[j, j] = np.sqrt(s)
            for i in range(j + 1, 6):
                s = M[i, j]
                for k in range(j):
                    s = s - L[i, k] * L[j, k]
                L[i, j] = s / L[j, j]
        y, x = np.zeros(6), np.zeros(6)
        for i in range(6):
            s = g[i]
            for k in range(i):
                s = s - L[i, k] * y[k]
            y[i] = s / L[i, i]
        for i in range(5, -1, -1):
            s = y[i]
            for k in range(i + 1, 6):
                s = s - L[k, i] * x[k]
            x[i] = s / L[i, i]
    return x, ok


def solve(sums, counts, damping=1e-3, lever_m=0.05, min_pixels=200):
    """(Q, 8) float64: omega, t, rms, solved."""
    Q = len(counts)
    out = np.zeros((Q, 8))
    for q in range(Q):
        used = int(counts[q, 6])
        M, g = matrix(sums[q], used, damping, lever_m)
        x, ok = cholesky_solve(M, g)
        ok = ok and used >= min_pixels
        out[q, :6] = x if ok else 0.0
        out[q, 6] = np.sqrt((np.float64(int(sums[q, 27])) * np.float64(2.0 ** -30)) / np.float64(used)) if used > 0 else np.nan
        out[q, 7] = 1.0 if ok else 0.0
    return out


def exp_so3(w):
    """Rodrigues' formula, fp64: (..., 3) -> (..., 3, 3); the series below 1e-8 rad."""
    w = np.asarray(w, np.float64)
    th = np.sqrt((w * w).sum(-1))[..., None, None]
    Kx = np.zeros(w.shape[:-1] + (3, 3))
    Kx[..., 0, 1], Kx[..., 0, 2], Kx[..., 1, 0] = -w[..., 2], w[..., 1], w[..., 2]
    Kx[..., 1, 2], Kx[..., 2, 0], Kx[..., 2, 1] = -w[..., 0], -w[..., 1], w[..., 0]
    small = th < 1e-8
    ths = np.where(small, 1.0, th)
    a = np.where(small, 1.0 - th * th / 6.0, np.sin(ths) / ths)
    b = np.where(small, 0.5 - th * th / 24.0, (1.0 - np.cos(ths)) / (ths * ths))
    return np.eye(3) + a * Kx + b * (Kx @ Kx)


def log_so3(R):
    """The rotation vector of one rotation matrix (3, 3), fp64, for angles below pi."""
    R = np.asarray(R, np.float64)
    w = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s, c = 0.5 * np.sqrt((w * w).sum()), 0.5 * (np.trace(R) - 1.0)
    th = np.arctan2(s, c)
    return 0.5 * w if s < 1e-10 else w * (th / (2.0 * s))


def rigid_step(R, pivot, placed, sol, max_rot_rad=0.5, max_shift_m=0.1):
    """One update of the rigid loop: (R', pivot', placed', applied (B,) bool), all fp64."""
    w, t = sol[:, :3], sol[:, 3:6]
    ok = (sol[:, 7] > 0.5) & (np.sqrt((w * w).sum(1)) <= max_rot_rad) & (np.sqrt((t * t).sum(1)) <= max_shift_m)
    E = exp_so3(w)
    R2 = E @ R
    moved = np.einsum("bij,bvj->bvi", E, placed - pivot[:, None, :]) + pivot[:, None, :] + t[:, None, :]
    return (np.where(ok[:, None, None], R2, R), np.where(ok[:, None], pivot + t, pivot),
            np.where(ok[:, None, None], moved, placed), ok)


def fit_rigid(render, vertices, cam_t, pivot, sensor, cameras, unit, ray_iterations=2, iterations=6, max_rot_rad=0.5,
              max_shift_m=0.1, gate_m=0.03, edge_m=0.005, reach_m=0.5, damping=1e-3, lever_m=0.05, min_pixels=200,
              raw_range=(1, 65535), ray_kw=None):
    """The rigid loop over ``render(placed (B, V, 3)) -> (depth, mesh_id)`` with mesh j the hand j: the ray rounds of
    depth_eval_rule.refine first (the pivot moves with the hand), then ``iterations`` rounds of fit + solve + rigid_step.
    Returns a dict: rotation, cam_t, pivot, rms, used, updated, and ``trail``: the placed vertices after the ray rounds and after
    every rigid round."""
    import depth_eval_rule as DR
    cam_t = np.asarray(cam_t)
    B = len(cam_t)
    ray = DR.refine(render, vertices, cam_t, sensor, unit, iterations=ray_iterations, raw_range=raw_range, **(ray_kw or {})) \
        if ray_iterations > 0 else (cam_t.copy(), None, None, np.zeros(B, bool), [])
    cam_ray = ray[0]
    pv = np.asarray(pivot, np.float64) + (cam_ray.astype(np.float64) - cam_t.astype(np.float64))
    placed = vertices.astype(np.float64) + cam_ray.astype(np.float64)[:, None, :]
    R = np.repeat(np.eye(3)[None], B, 0)
    shift = np.zeros((B, 3))
    any_step = np.zeros(B, bool)
    rms, used = np.full(B, np.nan), np.zeros(B, np.int64)
    trail = [placed.copy()]
    for _ in range(iterations):
        depth, mid = render(placed)
        sums, counts = fit(depth, mid, sensor, np.arange(B), B, cameras, pv, unit, gate_m, edge_m, reach_m, raw_range)
        sol = solve(sums, counts, damping, lever_m, min_pixels)
        R, pv2, placed, ok = rigid_step(R, pv, placed, sol, max_rot_rad, max_shift_m)
        shift = shift + (pv2 - pv)
        pv = pv2
        any_step |= ok
        rms, used = sol[:, 6], counts[:, 6]
        trail.append(placed.copy())
    out_t = np.where(any_step[:, None], (cam_ray.astype(np.float64) + shift).astype(cam_t.dtype), cam_ray)
    return {"rotation": R, "cam_t": out_t, "pivot": pv, "rms": rms, "used": used, "updated": ray[3] | any_step, "trail": trail}


def fold(pose_global, cam_t, R, cam_t_new, is_right):
    """A fit folded into a record: (pose_global' (3,), cam_t').  The record's mesh is M MANO(pose) + cam_t with M = diag(-1, 1, 1)
    for a left hand, and MANO turns the hand about its wrist joint, so the fitted rotation R about the placed wrist becomes the
    global orientation log(M R M exp(pose_global)) (M R M = R for a right hand)."""
    Mx = np.diag([1.0 if is_right else -1.0, 1.0, 1.0])
    Rg = exp_so3(np.asarray(pose_global, np.float64).reshape(3))
    return log_so3(Mx @ np.asarray(R, np.float64) @ Mx @ Rg), cam_t_new


def contraction_case(H=12, W=14):
    """A map on which a fused multiply-subtract in rz = raw * unit - d changes an integer of every used pixel: a flat patch
    at d = 0.5 seen by fx = fy = 512 (so n = (0, 0, 2^-18) and l2 = 2^-36 exactly and sums[26] adds llrint(rz * 2^30) per
    pixel), raw = 503, and ``unit`` the double nearest to (0.5 + (k + 0.5) 2^-30) / 503: raw * unit rounds to 0.5 +
    (k + 0.5) 2^-30 exactly, so the rule's rz * 2^30 is the tie k + 0.5 and goes to the even neighbour, while the unrounded
    product lies a little off the tie, on the odd neighbour's side (k is chosen so).  Returns (depth, pred_id, sensor, cameras,
    pivot, unit, plain, fused): the per-pixel integers of the rule and of a fused evaluation."""
    from fractions import Fraction
    for k in (3221225, 3221226, 3221227, 3221228):
        target = Fraction(1, 2) + Fraction(2 * k + 1, 2 ** 31)
        unit = float(target / 503)
        exact = Fraction(503) * Fraction(unit)
        if np.float64(503.0) * np.float64(unit) != float(target) or exact == target:
            continue
        plain = int(np.rint((np.float64(503.0) * np.float64(unit) - np.float64(0.5)) * SCALE))
        fused = int(np.rint(np.float64(float(exact - Fraction(1, 2))) * SCALE))            # exact - 0.5 is a double here: one rounding
        if plain != fused:
            break
    else:
        raise AssertionError("no k gives a tie")
    depth = np.full((1, H, W), 0.5, np.float32)
    pid = np.zeros((1, H, W), np.int32)
    sensor = np.full((1, H, W), 503, np.uint16)
    cameras = np.array([[512.0, 512.0, 7.0, 6.0]])
    return depth, pid, sensor, cameras, np.array([[0.0, 0.0, 0.5]]), unit, plain, fused
