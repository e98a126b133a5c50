"""The rule hm_mask_score is tested against (include/hamer_hip.h, "Mask scores"), in numpy: the
boundary map, the eight counts of one pred / gt pair by explicit dilation with a disk, and J, F, precision and recall from
counts.  Nothing here is shared with the kernel or with hamer/utils/mask_eval.py."""
import numpy as np

COUNT_NAMES = ("inter", "pred_area", "gt_area", "pred_boundary", "gt_boundary", "pred_matched", "gt_matched", "pixels")


def bmap(s):
    """b[y][x] = s differs from its east, south or south-east neighbour, the last row and column replicated."""
    s = np.asarray(s).astype(bool)
    e = np.concatenate([s[:, 1:], s[:, -1:]], 1)
    so = np.concatenate([s[1:], s[-1:]], 0)
    se = np.concatenate([so[:, 1:], so[:, -1:]], 1)
    return (s != e) | (s != so) | (s != se)


def bmap_assign_then_patch(s):
    """The other way the same map is written down: XOR with shifted copies whose last row / column stay zero, then the last
    row assigned again from the east copy alone, the last column from the south copy alone, and the bottom-right pixel cleared."""
    s = np.asarray(s).astype(bool)
    e, so, se = np.zeros_like(s), np.zeros_like(s), np.zeros_like(s)
    e[:, :-1] = s[:, 1:]
    so[:-1, :] = s[1:, :]
    se[:-1, :-1] = s[1:, 1:]
    b = (s ^ e) | (s ^ so) | (s ^ se)
    b[-1, :] = s[-1, :] ^ e[-1, :]
    b[:, -1] = s[:, -1] ^ so[:, -1]
    b[-1, -1] = False
    return b


def disk_offsets(r):
    r = int(r)
    return [(dy, dx) for dy in range(-r, r + 1) for dx in range(-r, r + 1) if dx * dx + dy * dy <= r * r]


def dilate(b, r):
    """b dilated by the disk of radius r: out[y][x] = some b[y + dy][x + dx] with dx dx + dy dy <= r r (outside the image: none)."""
    b = np.asarray(b).astype(bool)
    H, W = b.shape
    out = np.zeros_like(b)
    if not b.any():
        return out
    for dy, dx in disk_offsets(r):
        ys, yd = (slice(max(dy, 0), H + min(dy, 0)), slice(max(-dy, 0), H + min(-dy, 0)))
        xs, xd = (slice(max(dx, 0), W + min(dx, 0)), slice(max(-dx, 0), W + min(-dx, 0)))
        if ys.start < ys.stop and xs.start < xs.stop:
            out[yd, xd] |= b[ys, xs]
    return out


def counts(pred, gt, r):
    """The eight counts of one pair, int64."""
    pred, gt = np.asarray(pred).astype(bool), np.asarray(gt).astype(bool)
    bp, bg = bmap(pred), bmap(gt)
    return np.array([(pred & gt).sum(), pred.sum(), gt.sum(), bp.sum(), bg.sum(), (bp & dilate(bg, r)).sum(),
                     (bg & dilate(bp, r)).sum(), pred.size], np.int64)


def query_images(pred_id, mask, query):
    """(pred, gt) of one query (frame, id_lo, id_hi, label) on host arrays (N, H, W)."""
    f, lo, hi, label = (int(v) for v in query)
    pid, m = np.asarray(pred_id[f]).astype(np.int64), np.asarray(mask[f]).astype(np.int64)
    return (pid >= lo) & (pid < hi), (m != 0) if label == -1 else (m == label)


def query_counts(pred_id, mask, queries, r):
    """(Q, 8) int64; a query whose frame is outside the batch gives a row of zeros."""
    N = len(pred_id)
    rows = [counts(*query_images(pred_id, mask, q), r) if 0 <= int(q[0]) < N else np.zeros(8, np.int64) for q in queries]
    return np.stack(rows) if rows else np.zeros((0, 8), np.int64)


def jf(c):
    """(J, F, P, R) of one row of counts, Python floats (float64)."""
    inter, pa, ga, pb, gb, pm, gm = (int(v) for v in c[:7])
    J = 1.0 if pa + ga == 0 else inter / (pa + ga - inter)
    if pb == 0 and gb == 0:
        P, R = 1.0, 1.0
    elif pb == 0:
        P, R = 1.0, 0.0
    elif gb == 0:
        P, R = 0.0, 1.0
    else:
        P, R = pm / pb, gm / gb
    F = 0.0 if P + R == 0 else 2 * P * R / (P + R)
    return J, F, P, R


def blobs(H, W, seed, n=3):
    """A seeded binary image: the union of n random ellipses (some cut by the border)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    s = np.zeros((H, W), bool)
    for _ in range(n):
        cy, cx = rng.uniform(0, H), rng.uniform(0, W)
        ay, ax = rng.uniform(1, max(H / 3, 1.5)), rng.uniform(1, max(W / 3, 1.5))
        s |= ((yy - cy) / ay) ** 2 + ((xx - cx) / ax) ** 2 <= 1.0
    return s
