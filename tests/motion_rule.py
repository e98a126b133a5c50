"""The motion rule of include/hamer_hip.h ("Motion") and DESIGN.md section 10.8 in numpy: what hm_track_smooth and
hm_track_jitter (csrc/motion.hip) must equal byte for byte.  Not a test file.

Every expression below is one IEEE fp64 operation per numpy call, in the order the header states; nothing here is a library
routine except sqrt.  The functions are vectorised over (frame, track), which changes no value: every (frame, track) is
computed from its own window alone.
"""
import numpy as np

KEPT, SMOOTHED, FILLED, ABSENT, DEGENERATE = range(5)
MAX_RADIUS = 32
NEWTON_STEPS = 12
MIN_DET = 1.0 / 64.0
LANES = 64                                  # hm_track_jitter: one wave per (frame, track)


def window_weights(radius, sigma):
    """w[0] = 1, w[k] = exp(-0.5 (k / sigma)^2): hamer.utils.motion.window_weights restated."""
    k = np.arange(int(radius) + 1, dtype=np.float64)
    w = np.exp(-0.5 * (k / float(sigma)) ** 2)
    w[0] = 1.0
    return w


def cofactors(m):
    """The cofactor matrix of (..., 3, 3) and the determinant, in the header's order."""
    m00, m01, m02 = m[..., 0, 0], m[..., 0, 1], m[..., 0, 2]
    m10, m11, m12 = m[..., 1, 0], m[..., 1, 1], m[..., 1, 2]
    m20, m21, m22 = m[..., 2, 0], m[..., 2, 1], m[..., 2, 2]
    c = np.empty_like(m)
    c[..., 0, 0] = m11 * m22 - m12 * m21
    c[..., 0, 1] = m12 * m20 - m10 * m22
    c[..., 0, 2] = m10 * m21 - m11 * m20
    c[..., 1, 0] = m02 * m21 - m01 * m22
    c[..., 1, 1] = m00 * m22 - m02 * m20
    c[..., 1, 2] = m01 * m20 - m00 * m21
    c[..., 2, 0] = m01 * m12 - m02 * m11
    c[..., 2, 1] = m02 * m10 - m00 * m12
    c[..., 2, 2] = m00 * m11 - m01 * m10
    det = (m00 * c[..., 0, 0] + m01 * c[..., 0, 1]) + m02 * c[..., 0, 2]
    return c, det


def polar(m):
    """(rotation, degenerate) of the normalised sums m (..., 3, 3): degenerate where not det m >= 1/64, else 12 Newton steps
    X <- (X + cof(X) / det X) * 0.5.  The rotation of a degenerate entry means nothing."""
    with np.errstate(all="ignore"):
        _, det = cofactors(m)
        bad = ~(det >= MIN_DET)
        x = m.copy()
        for _ in range(NEWTON_STEPS):
            c, d = cofactors(x)
            x = (x + c / d[..., None, None]) * 0.5
    return x, bad


def track_smooth(rot, lin, present, w):
    """rot (N, S, J, 3, 3), lin (N, S, C) fp64, present (N, S) (non-zero: present), w (R + 1,) fp64.  Returns a dict: rot, lin
    (the shapes of the inputs), status, pairs, nearest_pair (N, S) int32 and moved (N, S, J) fp64."""
    rot = np.ascontiguousarray(rot, np.float64)
    lin = np.ascontiguousarray(lin, np.float64)
    w = np.asarray(w, np.float64)
    N, S, J = rot.shape[:3]
    R = len(w) - 1
    assert 0 <= R <= MAX_RADIUS and rot.shape[3:] == (3, 3) and lin.shape[:2] == (N, S)
    here = np.asarray(present).reshape(N, S) != 0
    nan = np.float64("nan")
    with np.errstate(all="ignore"):
        acc_r = np.where(here[:, :, None, None, None], w[0] * rot, 0.0)
        acc_l = np.where(here[:, :, None], w[0] * lin, 0.0)
        W = np.where(here, w[0], 0.0)
        pairs = np.zeros((N, S), np.int32)
        nearest = np.zeros((N, S), np.int32)
        for k in range(1, R + 1):
            pair = np.zeros((N, S), bool)
            if N > 2 * k:
                pair[k:N - k] = here[:N - 2 * k] & here[2 * k:]
            if not pair.any():
                continue
            sum_r = np.zeros_like(rot)
            sum_l = np.zeros_like(lin)
            sum_r[k:N - k] = rot[:N - 2 * k] + rot[2 * k:]              # A[t - k] + A[t + k]
            sum_l[k:N - k] = lin[:N - 2 * k] + lin[2 * k:]
            acc_r = np.where(pair[:, :, None, None, None], acc_r + w[k] * sum_r, acc_r)
            acc_l = np.where(pair[:, :, None], acc_l + w[k] * sum_l, acc_l)
            W = np.where(pair, W + 2.0 * w[k], W)
            nearest = np.where(pair & (pairs == 0), k, nearest).astype(np.int32)
            pairs += pair
        m = acc_r / W[:, :, None, None, None]
        x, bad = polar(m)
        lin_f = acc_l / W[:, :, None]
        any_pair = pairs > 0
        degenerate = any_pair & bad.any(axis=2)
        filtered = any_pair & ~degenerate
        status = np.where(here, KEPT, ABSENT)
        status = np.where(filtered, np.where(here, SMOOTHED, FILLED), status)
        status = np.where(degenerate, DEGENERATE, status).astype(np.int32)
        raw_r = np.where(here[:, :, None, None, None], rot, nan)
        raw_l = np.where(here[:, :, None], lin, nan)
        out_r = np.where(filtered[:, :, None, None, None], x, raw_r)
        out_l = np.where(filtered[:, :, None], lin_f, raw_l)
        moved = np.zeros((N, S, J), np.float64)
        for e in range(9):
            d = out_r[..., e // 3, e % 3] - rot[..., e // 3, e % 3]
            moved = moved + d * d
        moved = np.where((status == SMOOTHED)[:, :, None], moved, nan)
    # KEPT keeps the input's bytes, NaN payloads included
    keep = here & ~filtered
    out_r[keep] = rot[keep]
    out_l[keep] = lin[keep]
    return {"rot": out_r, "lin": out_l, "status": status, "pairs": pairs, "nearest_pair": nearest, "moved": moved}


def track_jitter(points, present):
    """points (N, S, P, 3) fp64, present (N, S).  accel (N, S) fp64: the mean over the points of |x[t-1] - 2 x[t] + x[t+1]|
    where t - 1, t, t + 1 are inside the sequence and present, NaN elsewhere.  Per point d = (x[t-1] - 2 x[t]) + x[t+1] per
    coordinate and n = sqrt((dx dx + dy dy) + dz dz); lane l of 64 adds the n of points l, l + 64, ... in this order to 0.0; the
    lanes meet as v[l] += v[l + o] for o = 32, 16, 8, 4, 2, 1; accel = v[0] / P."""
    x = np.ascontiguousarray(points, np.float64)
    N, S, P = x.shape[:3]
    here = np.asarray(present).reshape(N, S) != 0
    accel = np.full((N, S), np.nan)
    if N < 3 or P == 0:
        return accel
    with np.errstate(all="ignore"):
        d = (x[:-2] - 2.0 * x[1:-1]) + x[2:]
        n = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])      # (N - 2, S, P)
        rounds = (P + LANES - 1) // LANES
        padded = np.zeros((N - 2, S, rounds * LANES))
        padded[..., :P] = n
        v = np.zeros((N - 2, S, LANES))
        for r in range(rounds):
            v = v + padded[..., r * LANES:(r + 1) * LANES]
        o = LANES // 2
        while o:
            v = v[..., :o] + v[..., o:2 * o]
            o //= 2
        a = v[..., 0] / np.float64(P)
    ok = here[:-2] & here[1:-1] & here[2:]
    accel[1:-1] = np.where(ok, a, np.nan)
    return accel
