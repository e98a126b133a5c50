"""The skeleton drawing rule of include/hamer_hip.h (hm_skeleton_overlay) restated in numpy as a SEQUENTIAL painter: hand by
hand, primitive by primitive, every sample of a bone stamped with its disc -- independent of the kernel's per-pixel form.  At
line_radius 0, joint_radius 2 and interleaved order it is rootnet/Model_RGB.py draw_2d_skeleton."""
import numpy as np

INTERLEAVED, BONES_FIRST = 0, 1


def parent(j):
    return 0 if j % 4 == 1 else j - 1


def _offsets(r):
    return np.array([(dx, dy) for dy in range(-r, r + 1) for dx in range(-r, r + 1) if dx * dx + dy * dy <= r * r], np.int64)


def points(kp, threshold=0.1):
    """kp (21, 2 | 3) -> (int64 points (21, 2), present (21,) bool)."""
    kp = np.asarray(kp, np.float32)
    u, v = kp[:, 0].astype(np.float64), kp[:, 1].astype(np.float64)
    with np.errstate(invalid="ignore"):
        present = np.isfinite(u) & np.isfinite(v) & (np.abs(u) < 32768) & (np.abs(v) < 32768)
        if kp.shape[1] == 3:
            present &= kp[:, 2] > np.float32(threshold)
    pts = np.zeros((21, 2), np.int64)
    pts[present, 0] = np.trunc(u[present]).astype(np.int64)
    pts[present, 1] = np.trunc(v[present]).astype(np.int64)
    return pts, present


def draw_hand(img, kp, palette, line_radius, joint_radius, order=INTERLEAVED, threshold=0.1):
    """Draw one hand into img (H, W, 3) uint8 in place."""
    H, W = img.shape[:2]
    pts, present = points(kp, threshold)
    palette = np.asarray(palette, np.uint8).reshape(21, 3)
    line, disc = _offsets(int(line_radius)), _offsets(int(joint_radius))

    def stamp(sx, sy, offs, col):
        x = (np.asarray(sx, np.int64)[:, None] + offs[None, :, 0]).ravel()
        y = (np.asarray(sy, np.int64)[:, None] + offs[None, :, 1]).ravel()
        ok = (x >= 0) & (x < W) & (y >= 0) & (y < H)
        img[y[ok], x[ok]] = col

    def bone(j):
        q = parent(j)
        if not (present[j] and present[q]):
            return
        a, b = pts[q], pts[j]
        m = int(max(abs(b[0] - a[0]), abs(b[1] - a[1])))
        t = np.linspace(0.0, 1.0, m + 1)
        stamp(np.rint(a[0] + t * (b[0] - a[0])), np.rint(a[1] + t * (b[1] - a[1])), line, palette[j])

    def joint(j):
        if present[j]:
            stamp(pts[j:j + 1, 0], pts[j:j + 1, 1], disc, palette[j])

    if order == INTERLEAVED:
        for j in range(21):
            if j > 0:
                bone(j)
            joint(j)
    else:
        for j in range(1, 21):
            bone(j)
        for j in range(21):
            joint(j)
    return img


def draw(images, kp, hands, palette, order=INTERLEAVED):
    """images (N, H, W, 3) uint8, kp (n, 21, 2 | 3), hands [(image, line_radius, joint_radius, threshold)] -> a new array with
    every hand drawn, in table order."""
    out = np.array(images, np.uint8, copy=True)
    for i, (n, lr, jr, thr) in enumerate(hands):
        draw_hand(out[n], kp[i], palette, lr, jr, order, thr)
    return out
