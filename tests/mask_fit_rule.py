"""numpy restatement of the mask-fit rule (include/hamer_hip.h, "Mask fit"), the oracle of
tests/test_mask_fit_host.py and tests/test_gpu_mask_fit.py: the nearest-boundary match, the integer sums and counts, the damped
4 x 4 Cholesky solve, the similarity step of the contour loop and the loop itself.  Nothing here is shared with the kernel or
with hamer/utils/mask_eval.py.  Per-pixel work is integer; numpy never contracts a product and a sum and its fp64 division and
square root are IEEE, so every fp64 expression below is the rule's, in the rule's order."""
import numpy as np

from mask_eval_rule import bmap, query_images

SCALE = np.float64(2.0 ** 20)
PAIRS = [(i, j) for i in range(4) for j in range(i, 4)]                               # the 10 pairs, i <= j, row by row
N_SUMS = 18                                                                           # 10 pairs, 4 J_i, d2, anchors' ux, uy, uu
COUNT_NAMES = ("boundary", "matched", "anchored", "unmatched", "out_of_reach", "reserved5")
NO_MATCH = np.iinfo(np.int64).max


def disc_order(r):
    """The offsets (dx, dy) of the disc of radius r in the order the match prefers them: least d2, then least dy, then least dx."""
    r = int(r)
    offs = [(dx * dx + dy * dy, dy, dx) for dy in range(-r, r + 1) for dx in range(-r, r + 1) if dx * dx + dy * dy <= r * r]
    return [(dx, dy) for _, dy, dx in sorted(offs)]


def nearest(a, b, r):
    """For every set pixel of ``a`` (H, W) bool the nearest set pixel of ``b`` within the disc: (ys, xs, dx, dy, found), the
    pixels in row-major order."""
    a, b = np.asarray(a, bool), np.asarray(b, bool)
    H, W = a.shape
    ys, xs = np.nonzero(a)
    dx, dy = np.zeros(len(ys), np.int64), np.zeros(len(ys), np.int64)
    found = np.zeros(len(ys), bool)
    pad = np.zeros((H + 2 * r, W + 2 * r), bool)
    pad[r:r + H, r:r + W] = b
    if b.any():
        for ox, oy in disc_order(r):
            todo = np.nonzero(~found)[0]
            if not len(todo):
                break
            hit = todo[pad[ys[todo] + oy + r, xs[todo] + ox + r]]
            dx[hit], dy[hit], found[hit] = ox, oy, True
    return ys.astype(np.int64), xs.astype(np.int64), dx, dy, found


def terms(J, d2):
    """(n, 15) int64 of the point-to-line pixels: J (n, 4) int64, d2 (n,) int64 > 0."""
    out = np.zeros((len(d2), 15), np.int64)
    for k, (i, j) in enumerate(PAIRS):
        out[:, k] = np.rint((J[:, i] * J[:, j]).astype(np.float64) / d2.astype(np.float64) * SCALE).astype(np.int64)
    out[:, 10:14] = J
    out[:, 14] = d2
    return out


def pixels(pred, gt, centre, r, reach_px, direction):
    """One direction (1 or 2) of one query pixel by pixel: a dict of int64 arrays over the boundary pixels of its map A --
    ``found``, ``used``, ``d2``, the moved point ``u`` (n, 2) and the displacement ``d`` (n, 2) -- in row-major order."""
    bp, bg = bmap(pred), bmap(gt)
    ys, xs, dx, dy, found = nearest(bp, bg, r) if direction == 1 else nearest(bg, bp, r)
    cx, cy = int(centre[0]), int(centre[1])
    if direction == 1:
        ux, uy, ddx, ddy = xs - cx, ys - cy, dx, dy
    else:
        ux, uy, ddx, ddy = xs + dx - cx, ys + dy - cy, -dx, -dy
    near = (np.abs(ux) <= reach_px) & (np.abs(uy) <= reach_px)                        # so that the squares below cannot overflow
    uu = np.where(near, ux * ux + uy * uy, 0)
    reach = near & (uu <= int(reach_px) * int(reach_px))
    return {"found": found, "used": found & reach, "out": found & ~reach, "d2": dx * dx + dy * dy, "u": np.stack([ux, uy], 1),
            "d": np.stack([ddx, ddy], 1), "yx": np.stack([ys, xs], 1)}


def fit_pair(pred, gt, centre, r, reach_px, directions):
    """(sums (18,) int64, counts (2, 6) int64) of one pred / gt pair."""
    sums, counts = np.zeros(N_SUMS, np.int64), np.zeros((2, 6), np.int64)
    for k in (0, 1):
        if not (int(directions) >> k) & 1:
            continue
        p = pixels(pred, gt, centre, r, reach_px, k + 1)
        line, anchor = p["used"] & (p["d2"] > 0), p["used"] & (p["d2"] == 0)
        counts[k, :5] = len(p["found"]), line.sum(), anchor.sum(), (~p["found"]).sum(), p["out"].sum()
        u, d = p["u"][line], p["d"][line]
        J = np.stack([d[:, 0] * u[:, 0] + d[:, 1] * u[:, 1], -d[:, 0] * u[:, 1] + d[:, 1] * u[:, 0], d[:, 0], d[:, 1]], 1)
        sums[:15] += terms(J, p["d2"][line]).sum(0)
        ua = p["u"][anchor]
        sums[15:] += np.array([ua[:, 0].sum(), ua[:, 1].sum(), (ua * ua).sum()], np.int64)
    return sums, counts


def fit(pred_id, mask, queries, centre, r, reach_px, directions):
    """(sums (Q, 18), counts (Q, 2, 6)) int64 of host arrays (N, H, W); a query whose frame is outside the batch gives zeros."""
    Q, N = len(queries), len(pred_id)
    sums, counts = np.zeros((Q, N_SUMS), np.int64), np.zeros((Q, 2, 6), np.int64)
    for q, qu in enumerate(queries):
        if 0 <= int(qu[0]) < N:
            sums[q], counts[q] = fit_pair(*query_images(pred_id, mask, qu), centre[q], r, reach_px, directions)
    return sums, counts


def used_of(counts_q):
    c = np.asarray(counts_q).reshape(2, 6)
    return int(c[:, 1].sum() + c[:, 2].sum())


def matrix(sums_q, counts_q, damping, lever_px):
    """(M (4, 4), g (4,)) of one query's integers, every addition in the header's order."""
    f = np.float64
    inv = f(2.0 ** -20)
    s = [int(v) for v in sums_q]
    c = np.asarray(counts_q).reshape(2, 6)
    M, g = np.zeros((4, 4)), np.zeros(4)
    for k, (i, j) in enumerate(PAIRS):
        M[i, j] = M[j, i] = f(s[k]) * inv
    na, sx, sy, suu = f(int(c[0, 2] + c[1, 2])), f(s[15]), f(s[16]), f(s[17])
    M[0, 0] = M[0, 0] + suu
    M[1, 1] = M[1, 1] + suu
    M[0, 2] = M[2, 0] = M[0, 2] + sx
    M[0, 3] = M[3, 0] = M[0, 3] + sy
    M[1, 2] = M[2, 1] = M[1, 2] - sy
    M[1, 3] = M[3, 1] = M[1, 3] + sx
    M[2, 2] = M[2, 2] + na
    M[3, 3] = M[3, 3] + na
    du = f(damping) * f(used_of(c))
    lever2 = f(lever_px) * f(lever_px)
    for i in (0, 1):
        M[i, i] = M[i, i] + du * lever2
    for i in (2, 3):
        M[i, i] = M[i, i] + du
    for i in range(4):
        g[i] = f(s[10 + i])
    return M, g


def cholesky_solve(M, g):
    """(x, every pivot > 0) in hm_depth_fit's order for n = 4: column by column, inner sums from k = 0 upwards."""
    n = 4
    L = np.zeros((n, n))
    ok = True
    with np.errstate(all="ignore"):
        for j in range(n):
            s = M[j, j]
            for k in range(j):
                s = s - L[j, k] * L[j, k]
            if not s > 0.0:
                ok = False
            L[j, j] = np.sqrt(s)
            for i in range(j + 1, n):
                s = M[i, j]
                for k in range(j):
                    s = s - L[i, k] * L[j, k]
                L[i, j] = s / L[j, j]
        y, x = np.zeros(n), np.zeros(n)
        for i in range(n):
            s = g[i]
            for k in range(i):
                s = s - L[i, k] * y[k]
            y[i] = s / L[i, i]
        for i in range(n - 1, -1, -1):
            s = y[i]
            for k in range(i + 1, n):
                s = s - L[k, i] * x[k]
            x[i] = s / L[i, i]
    return x, ok


def solve(sums, counts, damping=1e-3, lever_px=50.0, min_pixels=30):
    """(Q, 8) float64: alpha, beta, tx, ty, rms, solved, 0, 0."""
    Q = len(sums)
    out = np.zeros((Q, 8))
    for q in range(Q):
        used = used_of(counts[q])
        M, g = matrix(sums[q], counts[q], damping, lever_px)
        x, ok = cholesky_solve(M, g)
        ok = ok and used >= min_pixels
        out[q, :4] = x if ok else 0.0
        out[q, 4] = np.sqrt(np.float64(int(sums[q][14])) / np.float64(used)) if used > 0 else 0.0
        out[q, 5] = 1.0 if ok else 0.0
    return out


# ---------------------------------------------------------------------------------------------------------------- the loop
def exp_so3(w):
    """Rodrigues' formula, fp64: (B, 3) -> (B, 3, 3); the series below 1e-8 rad."""
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


def project(cams, frame_index, pivot):
    """(B, 2) float64: the real-valued pixel of each pivot (B, 3) under its frame's fx, fy, cx, cy."""
    c = np.asarray(cams, np.float64)[np.asarray(frame_index)]
    return np.stack([c[:, 0] * pivot[:, 0] / pivot[:, 2] + c[:, 2], c[:, 1] * pivot[:, 1] / pivot[:, 2] + c[:, 3]], 1)


def centre_of(proj):
    """The integer pixel nearest to a projection (ties to even, as rint)."""
    return np.rint(proj).astype(np.int64)


def contour_step(R, pivot, placed, sol, centre, cams, frame_index, radius, max_rot_rad=0.5, max_scale=2.0):
    """One update of the contour loop: (R', pivot', placed', applied (B,) bool), all fp64.  The similarity about ``centre``
    moves the pivot's projection, the scale divides its depth, and the in-plane angle turns the hand about the pivot's ray."""
    al, be, t = sol[:, 0], sol[:, 1], sol[:, 2:4]
    s, phi = np.hypot(1.0 + al, be), np.arctan2(be, 1.0 + al)
    ok = (sol[:, 5] > 0.5) & (np.abs(phi) <= max_rot_rad) & (s >= 1.0 / max_scale) & (s <= max_scale) \
        & (np.sqrt((t * t).sum(1)) <= float(radius))
    c = np.asarray(cams, np.float64)[np.asarray(frame_index)]
    p = project(cams, frame_index, pivot)
    v = p - centre
    p2 = centre + (1.0 + al)[:, None] * v + be[:, None] * np.stack([-v[:, 1], v[:, 0]], 1) + t
    z2 = pivot[:, 2] / s
    pv2 = np.stack([(p2[:, 0] - c[:, 2]) / c[:, 0] * z2, (p2[:, 1] - c[:, 3]) / c[:, 1] * z2, z2], 1)
    ray = pivot / np.sqrt((pivot * pivot).sum(1))[:, None]
    E = exp_so3(phi[:, None] * ray)
    moved = np.einsum("bij,bvj->bvi", E, placed - pivot[:, None, :]) + pv2[:, None, :]
    return (np.where(ok[:, None, None], E @ R, R), np.where(ok[:, None], pv2, pivot), np.where(ok[:, None, None], moved, placed), ok)


def fit_contour(render, vertices, cam_t, pivot, frame_index, mask, labels, cams, rounds=6, radius=8, reach_px=4096,
                damping=1e-3, lever_px=50.0, min_pixels=30, directions=None):
    """The contour loop over ``render(placed (B, V, 3)) -> mesh_id (N, H, W)`` with mesh j the hand j.  Returns a dict:
    rotation, cam_t, pivot, rms, pixels, fitted, and ``trail``: the placed vertices at the start and after every round."""
    cam_t = np.asarray(cam_t)
    B = len(cam_t)
    pv = np.asarray(pivot, np.float64).copy()
    placed = np.asarray(vertices, np.float64) + cam_t.astype(np.float64)[:, None, :]
    R = np.repeat(np.eye(3)[None], B, 0)
    if directions is None:
        pairs = [(int(f), int(l)) for f, l in zip(frame_index, labels)]
        directions = [1 if pairs.count(p) > 1 else 3 for p in pairs]
    fitted = np.zeros(B, bool)
    rms, pix = np.zeros(B), np.zeros(B, np.int64)
    trail = [placed.copy()]
    pv0 = pv.copy()
    for _ in range(rounds):
        mid = render(placed)
        centre = centre_of(project(cams, frame_index, pv))
        sol = np.zeros((B, 8))
        for j in range(B):
            sums, counts = fit(mid, mask, [(frame_index[j], j, j + 1, labels[j])], centre[j:j + 1], radius, reach_px, directions[j])
            sol[j] = solve(sums, counts, damping, lever_px, min_pixels)[0]
            pix[j] = used_of(counts[0])
        R, pv, placed, ok = contour_step(R, pv, placed, sol, centre.astype(np.float64), cams, frame_index, radius)
        fitted |= ok
        rms = sol[:, 4]
        trail.append(placed.copy())
    out_t = np.where(fitted[:, None], (cam_t.astype(np.float64) + (pv - pv0)).astype(cam_t.dtype), cam_t)
    return {"rotation": R, "cam_t": out_t, "pivot": pv, "rms": rms, "pixels": pix, "fitted": fitted, "trail": trail}


# ---------------------------------------------------------------------------------------------------------------- shapes
def tie_shapes():
    """Three (pred, gt) pairs, 10 x 12, in which the pred boundary pixel (4, 5) lies midway between gt boundary pixels: (4, 2)
    and (4, 8); (1, 5) and (7, 5); and the four of (1 or 7, 2 or 8).  Single pixels: a lone set pixel at (y, x) makes the block
    (y-1 .. y, x-1 .. x) boundary pixels, so a block right of or below (4, 5) is set one pixel further out."""
    out = []
    for (py, px), gts in (((4, 5), [(4, 2), (4, 9)]), ((4, 5), [(1, 5), (8, 5)]), ((4, 5), [(1, 2), (8, 9), (1, 9), (8, 2)])):
        pred, gt = np.zeros((10, 12), bool), np.zeros((10, 12), bool)
        pred[py, px] = True
        for y, x in gts:
            gt[y, x] = True
        out.append((pred, gt))
    return out
