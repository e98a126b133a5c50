"""The interpenetration rule of include/hamer_hip.h ("Penetration") in numpy: integers and float64, every expression in the
header's order, so hm_mesh_penetration can equal it bit for bit.  A query is an ordered pair of meshes (a, b): every vertex of a
gets its signed distance to the surface of b.  ``close_boundaries`` and the measure-then-move loop are restated here as well;
the package's own copies live in hamer/utils/penetration.py."""
import math

import numpy as np

FAR, NEAR, INSIDE, INVALID = 0, 1, 2, 3
OK, DISJOINT, TOO_LARGE = 0, 1, 2
TESTED, N_NEAR, N_INSIDE, N_INVALID, STATUS, MAX_BITS, SUM_DEPTH, PUSH_X, PUSH_Y, PUSH_Z = range(10)
QUANTA = 65536.0                       # per metre
SIDE_LIMIT = 1 << 17                   # a box side of 2 m
COORD_LIMIT = 16384.0                  # |coordinate| < 2^14 m, so |X| <= 2^30
I32_MAX, I32_MIN = 2 ** 31 - 1, -2 ** 31


def quantise(verts):
    """(X (n, 3) int64, valid (n,)): X = rint_half_even(x * 2^16); a vertex is valid when every coordinate is finite and
    |x| < 16384."""
    v = np.asarray(verts, np.float64).reshape(-1, 3)
    with np.errstate(invalid="ignore"):
        valid = (np.abs(v) < COORD_LIMIT).all(1)                         # NaN and inf compare false
    X = np.zeros(v.shape, np.int64)
    X[valid] = np.rint(v[valid] * QUANTA).astype(np.int64)
    return X, valid


def tol_quanta(contact_tol_m):
    return int(math.ceil(float(contact_tol_m) * QUANTA))


def box_of(X, valid):
    if not valid.any():
        return np.full(3, I32_MAX, np.int64), np.full(3, I32_MIN, np.int64)
    return X[valid].min(0), X[valid].max(0)


def _owns(ax, ay, bx, by):
    dy, dx = by - ay, bx - ax
    return (dy < 0) | ((dy == 0) & (dx > 0))


def prepare_faces(X, valid, faces):
    """The faces of b as the kernel stages them: (ok (F,), V (F, 3, 3) int64 corners with 1 and 2 swapped where the projected
    area A is negative, own (F, 3) ownership of the edges opposite corner 0, 1, 2, A (F,) >= 0, n (F, 3) integer normal)."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    nv = len(X)
    in_range = ((f >= 0) & (f < nv)).all(1)
    fc = np.where(in_range[:, None], f, 0) if nv else np.zeros_like(f)
    ok = in_range & (valid[fc].all(1) if nv else np.zeros(len(f), bool))
    V = X[fc] if nv else np.zeros((len(f), 3, 3), np.int64)
    V = np.where(ok[:, None, None], V, 0)
    A = (V[:, 1, 0] - V[:, 0, 0]) * (V[:, 2, 1] - V[:, 0, 1]) - (V[:, 1, 1] - V[:, 0, 1]) * (V[:, 2, 0] - V[:, 0, 0])
    swap = A < 0
    V[swap] = V[swap][:, [0, 2, 1]]
    A = np.abs(A)
    own = np.stack([_owns(V[:, 1, 0], V[:, 1, 1], V[:, 2, 0], V[:, 2, 1]), _owns(V[:, 2, 0], V[:, 2, 1], V[:, 0, 0], V[:, 0, 1]),
                    _owns(V[:, 0, 0], V[:, 0, 1], V[:, 1, 0], V[:, 1, 1])], 1)
    ab, ac = V[:, 1] - V[:, 0], V[:, 2] - V[:, 0]
    n = np.stack([ab[:, 1] * ac[:, 2] - ab[:, 2] * ac[:, 1], ab[:, 2] * ac[:, 0] - ab[:, 0] * ac[:, 2],
                  ab[:, 0] * ac[:, 1] - ab[:, 1] * ac[:, 0]], 1)
    return ok, V, own, A, n


def _edge(ax, ay, bx, by, px, py):
    return (bx - ax) * (py - ay) - (by - ay) * (px - ax)


def crossings(P, ok, V, own, A, n):
    """(m, F) bool: face f is crossed by the ray from P[i] in +z."""
    px, py = P[:, None, 0], P[:, None, 1]
    e0 = _edge(V[:, 1, 0], V[:, 1, 1], V[:, 2, 0], V[:, 2, 1], px, py)
    e1 = _edge(V[:, 2, 0], V[:, 2, 1], V[:, 0, 0], V[:, 0, 1], px, py)
    e2 = _edge(V[:, 0, 0], V[:, 0, 1], V[:, 1, 0], V[:, 1, 1], px, py)
    cov = lambda e, o: (e > 0) | ((e == 0) & o)                          # noqa: E731
    inside_xy = cov(e0, own[:, 0]) & cov(e1, own[:, 1]) & cov(e2, own[:, 2])
    e = V[None, :, 0, :] - P[:, None, :]
    s = n[None, :, 0] * e[..., 0] + n[None, :, 1] * e[..., 1] + n[None, :, 2] * e[..., 2]      # int64, exact
    return inside_xy & (s > 0) & (ok & (A != 0))[None, :]


def deltas(P, V, n):
    """(m, F, 3) float64, in quanta: closest point of face f minus P[i], by the region method in the header's order."""
    f8 = np.float64
    a, b, c = V[None, :, 0, :], V[None, :, 1, :], V[None, :, 2, :]
    p = P[:, None, :]
    ab, ac, bc = (b - a), (c - a), (c - b)
    ap, bp, cp = p - a, p - b, p - c
    dot = lambda u, w: (u[..., 0] * w[..., 0] + u[..., 1] * w[..., 1] + u[..., 2] * w[..., 2]).astype(f8)   # noqa: E731  exact
    d1, d2, d3, d4, d5, d6 = dot(ab, ap), dot(ac, ap), dot(ab, bp), dot(ac, bp), dot(ab, cp), dot(ac, cp)
    abf, acf, bcf, apf, bpf, cpf = (np.broadcast_to(x, ap.shape).astype(f8) for x in (ab, ac, bc, ap, bp, cp))
    nf = np.broadcast_to(n[None].astype(f8), ap.shape)
    out = np.zeros(ap.shape, f8)
    left = np.ones(ap.shape[:2], bool)

    def take(cond, value):
        nonlocal left
        sel = left & cond
        out[sel] = value[sel]
        left = left & ~sel

    with np.errstate(divide="ignore", invalid="ignore"):
        take((d1 <= 0) & (d2 <= 0), -apf)
        take((d3 >= 0) & (d4 <= d3), -bpf)
        vc = d1 * d4 - d3 * d2
        v = d1 / (d1 - d3)
        take((vc <= 0) & (d1 >= 0) & (d3 <= 0), v[..., None] * abf - apf)
        take((d6 >= 0) & (d5 <= d6), -cpf)
        vb = d5 * d2 - d1 * d6
        w = d2 / (d2 - d6)
        take((vb <= 0) & (d2 >= 0) & (d6 <= 0), w[..., None] * acf - apf)
        va = d3 * d6 - d5 * d4
        w = (d4 - d3) / ((d4 - d3) + (d5 - d6))
        take((va <= 0) & ((d4 - d3) >= 0) & ((d5 - d6) >= 0), w[..., None] * bcf - bpf)
        nn = (nf[..., 0] * nf[..., 0] + nf[..., 1] * nf[..., 1]) + nf[..., 2] * nf[..., 2]
        s = (nf[..., 0] * -apf[..., 0] + nf[..., 1] * -apf[..., 1]) + nf[..., 2] * -apf[..., 2]
        t = s / nn
        take(np.ones_like(left), nf * t[..., None])
    return out


def query(verts_a, verts_b, faces_b, contact_tol_m=0.002):
    """One query.  Returns {'code' (na,) u8, 'signed_distance' (na,) f32, 'nearest_face' (na,) i32, 'sums' (10,) i64,
    'delta' (na, 3) f64 quanta (closest point minus vertex, 0 where there is no distance)}."""
    Xa, va = quantise(verts_a)
    Xb, vb = quantise(verts_b)
    na = len(Xa)
    T = tol_quanta(contact_tol_m)
    code = np.where(va, FAR, INVALID).astype(np.uint8)
    sd = np.where(va, np.inf, np.nan).astype(np.float32)
    near = np.full(na, -1, np.int32)
    sums = np.zeros(10, np.int64)
    delta = np.zeros((na, 3), np.float64)
    out = {"code": code, "signed_distance": sd, "nearest_face": near, "sums": sums, "delta": delta}
    alo, ahi = box_of(Xa, va)
    blo, bhi = box_of(Xb, vb)
    if ((ahi - alo) >= SIDE_LIMIT).any() or ((bhi - blo) >= SIDE_LIMIT).any():
        code[:] = INVALID
        sd[:] = np.nan
        sums[STATUS] = TOO_LARGE
        return out
    sums[N_INVALID] = int((~va).sum())
    if not ((alo <= bhi + T) & (blo - T <= ahi)).all():
        sums[STATUS] = DISJOINT
        return out
    tested = va & ((Xa >= blo - T) & (Xa <= bhi + T)).all(1)
    sums[TESTED] = int(tested.sum())
    idx = np.nonzero(tested)[0]
    ok, V, own, A, n = prepare_faces(Xb, vb, faces_b)
    use = ok & (n != 0).any(1)                                           # faces of area 0 in space give no distance
    if len(idx) == 0 or len(V) == 0:
        return out
    P = Xa[idx]
    odd = (crossings(P, ok, V, own, A, n).sum(1) & 1).astype(bool)
    D = deltas(P, V, n)
    d2 = (D[..., 0] * D[..., 0] + D[..., 1] * D[..., 1]) + D[..., 2] * D[..., 2]
    d2 = np.where(use[None, :], d2, np.inf)
    best = d2.argmin(1)                                                  # the first minimum: ties go to the lower face row
    d2min = d2[np.arange(len(idx)), best]
    d = np.sqrt(d2min) * (1.0 / QUANTA)                                  # metres, float64
    for k, i in enumerate(idx):
        if odd[k]:
            code[i], sd[i], near[i], delta[i] = INSIDE, np.float32(-d[k]), best[k], D[k, best[k]]
            sums[N_INSIDE] += 1
            sums[MAX_BITS] = max(int(sums[MAX_BITS]), int(np.float64(d[k]).view(np.int64)))
            sums[SUM_DEPTH] += int(np.rint(d[k] * 4294967296.0))
            sums[PUSH_X:PUSH_Z + 1] += np.rint(D[k, best[k]] * QUANTA).astype(np.int64)
        elif d[k] <= contact_tol_m:
            code[i], sd[i], near[i], delta[i] = NEAR, np.float32(d[k]), best[k], D[k, best[k]]
            sums[N_NEAR] += 1
    return out


def max_depth(sums):
    """The maximum penetration depth in metres of one query's sums, or of a (Q, 10) array of them."""
    return np.asarray(sums, np.int64)[..., MAX_BITS].copy().view(np.float64)


def close_boundaries(faces, n_verts):
    """The faces that close the holes of a mesh: the boundary edges (used by exactly one face) are chained into loops, and each
    loop is fanned from its lowest-index vertex, against the direction its faces run, so the fans face outward with the rest.
    (K, 3) int32; no vertex is added."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    if len(f) and (f.min() < 0 or f.max() >= n_verts):
        raise ValueError("close_boundaries: a corner index outside the vertices")
    directed = {}
    for a, b in np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]).tolist():
        directed[(a, b)] = directed.get((a, b), 0) + 1
    nxt = {}
    for (a, b), k in directed.items():
        if k + directed.get((b, a), 0) == 1:
            if b in nxt:
                raise ValueError("close_boundaries: two boundary loops touch at a vertex")
            nxt[b] = a                                                   # the closing faces run b -> a
    extra = []
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


def resolve(verts, faces, pairs, rounds=8, gain=1.125, contact_tol_m=0.002):
    """The measure-then-move loop of hamer.utils.penetration.resolve_penetration on lists of vertex arrays and face arrays:
    (shift (n, 3) float64 metres, the (len(pairs), 2, 10) sums measured after the last move)."""
    n = len(verts)
    tq = np.zeros((n, 3), np.int64)
    for _ in range(rounds):
        moved = [np.asarray(v, np.float64) + tq[i] * (1.0 / QUANTA) for i, v in enumerate(verts)]
        step = np.zeros((n, 3), np.int64)
        for i, j in pairs:
            s1 = query(moved[i], moved[j], faces[j], contact_tol_m)["sums"]
            s2 = query(moved[j], moved[i], faces[i], contact_tol_m)["sums"]
            D = (s1[PUSH_X:PUSH_Z + 1] - s2[PUSH_X:PUSH_Z + 1]).astype(np.float64)
            norm = np.sqrt((D[0] * D[0] + D[1] * D[1]) + D[2] * D[2])
            length = gain * max(max_depth(s1), max_depth(s2))
            if s1[N_INSIDE] + s2[N_INSIDE] > 0 and norm > 0:
                half = np.rint(D / norm * (length * 0.5) * QUANTA).astype(np.int64)
                step[i] += half
                step[j] -= half
        tq += step
    moved = [np.asarray(v, np.float64) + tq[i] * (1.0 / QUANTA) for i, v in enumerate(verts)]
    last = np.stack([np.stack([query(moved[i], moved[j], faces[j], contact_tol_m)["sums"],
                               query(moved[j], moved[i], faces[i], contact_tol_m)["sums"]]) for i, j in pairs]) if pairs else np.zeros((0, 2, 10), np.int64)
    return tq * (1.0 / QUANTA), last
