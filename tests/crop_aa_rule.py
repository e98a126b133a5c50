"""The rule of the anti-aliased HaMeR crop (``hamer_inference.prepare_item``, hamer/infer.py:263-352) restated in numpy, in
fp64 (the truth the GPU tests compare with) and, by ``dtype=np.float32``, in fp32 (how far plain fp32 arithmetic lands from it).
Built on ``oracle.crop_ref`` for the box arithmetic, the affine map and the coordinate arithmetic of ``warp_affine_u8``.

The steps (infer.py:314-339):
  * ``df = (S / P) / 2``; ``df <= 1.1``: the crop of ``prepare_batch_bbox``, the 8-bit warp -- ``crop_ref.prepare_batch_bbox``;
  * else ``sigma = (df - 1) / 2`` and the frame becomes ``skimage.filters.gaussian(img, sigma, channel_axis=2,
    preserve_range=True)``: a float image, per axis ``radius = int(4 sigma + 0.5)`` normalised taps ``exp(-k^2 / (2 sigma^2))``
    over replicated edges, channels apart, nothing rounded;
  * ``cv2.warpAffine(INTER_LINEAR, BORDER_CONSTANT 0)`` of the float image: the source coordinates of the 8-bit path (10-bit
    fixed point, ``round_delta`` 16, 1/32 px), the four taps blended with ``(32-fx)(32-fy)/1024`` ... in floating point, a tap
    outside the frame counting 0, no rounding;
  * BGR -> RGB, mirror for a left hand, ``(v - mean_c) / std_c`` with the fp32 mean and std the kernels are handed.

PARITY UNPINNED against scikit-image and OpenCV, neither of which is installed here.  ``skimage.filters.gaussian`` hands its
work to ``scipy.ndimage.gaussian_filter(img, (sigma, sigma, 0), mode='nearest', truncate=4.0)``, which IS installed, so scipy
is the oracle of the blur (tests/test_crop_aa_host.py compares ``gaussian_blur`` with it).  The float warp restates the
non-8-bit path of ``cv::warpAffine`` by the same hypothesis ``oracle/crop_ref.py`` states for the 8-bit one -- the same
coordinate tables, floating-point weights from the same 1/32-px table; it cannot be verified without cv2.
"""
from __future__ import annotations

import math

import numpy as np

from oracle import crop_ref

AB_BITS, INTER_BITS, INTER_TAB = crop_ref.AB_BITS, crop_ref.INTER_BITS, crop_ref.INTER_TAB
MAX_RADIUS = 48


def blur_of_size(S: float, P: int = 256):
    """(sigma, radius) of a crop of side S, or None on the 8-bit path (df <= 1.1)."""
    df = (S / P) / 2.0
    if not df > 1.1:
        return None
    sigma = (df - 1) / 2
    return sigma, int(4.0 * sigma + 0.5)


def gaussian_taps(sigma: float, radius: int) -> np.ndarray:
    """scipy.ndimage's _gaussian_kernel1d: taps k = -radius .. radius in double, normalised to sum 1."""
    c = -0.5 / (sigma * sigma)
    phi = [math.exp(c * float(k * k)) for k in range(-radius, radius + 1)]
    total = 0.0
    for v in phi:
        total += v
    return np.array([v / total for v in phi], dtype=np.float64)


def gaussian_blur_at(img: np.ndarray, sigma: float, radius: int, rows: np.ndarray, cols: np.ndarray, dtype=np.float64) -> np.ndarray:
    """Rows ``rows`` and columns ``cols`` (index arrays inside the frame) of gaussian_filter(img, (sigma, sigma, 0),
    mode='nearest', truncate=4.0), computed in ``dtype``: axis 0 first, then axis 1, as scipy goes, each a running sum over the
    taps in ascending order.  (A crop reads at most 2 P rows and 2 P columns of the blurred frame; the rest is never formed.)"""
    g = gaussian_taps(sigma, radius).astype(dtype)
    H, W = img.shape[:2]
    a = img.astype(dtype)
    v = np.zeros((len(rows), W, 3), dtype)
    for k in range(2 * radius + 1):
        v = v + g[k] * a[np.clip(rows + (k - radius), 0, H - 1)]
    h = np.zeros((len(rows), len(cols), 3), dtype)
    for k in range(2 * radius + 1):
        h = h + g[k] * v[:, np.clip(cols + (k - radius), 0, W - 1)]
    return h


def gaussian_blur(img: np.ndarray, sigma: float, radius: int, dtype=np.float64) -> np.ndarray:
    """The whole blurred frame."""
    return gaussian_blur_at(img, sigma, radius, np.arange(img.shape[0]), np.arange(img.shape[1]), dtype)


def warp_coords(M: np.ndarray, out_w: int, out_h: int):
    """The integer source coordinates and 1/32-px fractions of crop_ref.warp_affine_u8: (sx, sy, fx, fy), each (out_h, out_w)."""
    M = np.array(M, dtype=np.float64)
    D = M[0, 0] * M[1, 1] - M[0, 1] * M[1, 0]
    D = 1.0 / D if D != 0 else 0.0
    iM = np.array([[M[1, 1] * D, -M[0, 1] * D, 0.0], [-M[1, 0] * D, M[0, 0] * D, 0.0]])
    iM[0, 2] = -iM[0, 0] * M[0, 2] - iM[0, 1] * M[1, 2]
    iM[1, 2] = -iM[1, 0] * M[0, 2] - iM[1, 1] * M[1, 2]
    xs, ys = np.arange(out_w, dtype=np.float64), np.arange(out_h, dtype=np.float64)
    AB = float(1 << AB_BITS)
    adelta = np.rint(iM[0, 0] * xs * AB).astype(np.int64)
    bdelta = np.rint(iM[1, 0] * xs * AB).astype(np.int64)
    rd = (1 << AB_BITS) // INTER_TAB // 2
    X0 = np.rint((iM[0, 1] * ys + iM[0, 2]) * AB).astype(np.int64) + rd
    Y0 = np.rint((iM[1, 1] * ys + iM[1, 2]) * AB).astype(np.int64) + rd
    X = (X0[:, None] + adelta[None, :]) >> (AB_BITS - INTER_BITS)
    Y = (Y0[:, None] + bdelta[None, :]) >> (AB_BITS - INTER_BITS)
    return X >> INTER_BITS, Y >> INTER_BITS, X & (INTER_TAB - 1), Y & (INTER_TAB - 1)


def warp_affine_float(img: np.ndarray, M: np.ndarray, out_w: int, out_h: int, dtype=np.float64, blur=None) -> np.ndarray:
    """cv::warpAffine, float image, INTER_LINEAR, BORDER_CONSTANT(0): warp_affine_u8's taps, blended in ``dtype``, unrounded.
    ``blur = (sigma, radius)``: the image sampled is the blurred frame, formed only where the taps read it."""
    sx, sy, fx, fy = warp_coords(M, out_w, out_h)
    H, W = img.shape[:2]
    rows = np.unique(np.clip(np.concatenate([sy[:, 0], sy[:, 0] + 1]), 0, H - 1))
    cols = np.unique(np.clip(np.concatenate([sx[0], sx[0] + 1]), 0, W - 1))
    src = img.astype(dtype)[rows][:, cols] if blur is None else gaussian_blur_at(img, blur[0], blur[1], rows, cols, dtype)

    def tap(yy, xx):
        ok = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
        v = src[np.searchsorted(rows, np.clip(yy, 0, H - 1)), np.searchsorted(cols, np.clip(xx, 0, W - 1))]
        return v * ok[..., None].astype(dtype)

    q = dtype(1.0 / (INTER_TAB * INTER_TAB))                    # (the weights k / 1024 are exact in either format)
    w00 = (((INTER_TAB - fx) * (INTER_TAB - fy)).astype(dtype) * q)[..., None]
    w01 = ((fx * (INTER_TAB - fy)).astype(dtype) * q)[..., None]
    w10 = (((INTER_TAB - fx) * fy).astype(dtype) * q)[..., None]
    w11 = ((fx * fy).astype(dtype) * q)[..., None]
    return w00 * tap(sy, sx) + w01 * tap(sy, sx + 1) + w10 * tap(sy + 1, sx) + w11 * tap(sy + 1, sx + 1)


def interior_mask(M: np.ndarray, out_w: int, out_h: int, H: int, W: int, radius: int) -> np.ndarray:
    """(out_h, out_w) bool, before any mirror: the four taps and their whole blur support lie inside the frame."""
    sx, sy, _, _ = warp_coords(M, out_w, out_h)
    return (sx - radius >= 0) & (sx + 1 + radius < W) & (sy - radius >= 0) & (sy + 1 + radius < H)


def prepare_item_img(img_bgr: np.ndarray, bbox, mean, std, bbox_shape=(192, 256), image_size=256, dtype=np.float64) -> np.ndarray:
    """``prepare_item(img_bgr, bbox)['img'][0]``: (3, P, P) in ``dtype`` (the 8-bit path returns its fp32 values in it)."""
    label, (x1, y1, x2, y2) = bbox
    P = image_size
    cx, cy, S = crop_ref.bbox_to_center_size(x1, y1, x2, y2, bbox_shape)
    blur = blur_of_size(S, P)
    if blur is None:
        return crop_ref.prepare_batch_bbox(img_bgr, [bbox], mean, std, bbox_shape, P)["img"][0].astype(dtype)
    sigma, radius = blur
    trans = crop_ref.gen_trans_from_patch(cx, cy, S, S, P, P)
    patch = warp_affine_float(img_bgr, trans, P, P, dtype, blur=(sigma, radius))
    patch = patch[:, :, ::-1]
    if label != "right":
        patch = patch[:, ::-1]
    t = np.transpose(patch, (2, 0, 1)).astype(dtype)
    out = np.empty_like(t)
    for c in range(3):
        out[c] = (t[c] - dtype(np.float32(mean[c]))) / dtype(np.float32(std[c]))
    return out


def prepare_items(img_bgr: np.ndarray, bboxs, mean, std, dtype=np.float64, **kw) -> np.ndarray:
    return np.stack([prepare_item_img(img_bgr, b, mean, std, dtype=dtype, **kw) for b in bboxs])


def is_blurred(bbox, bbox_shape=(192, 256), image_size=256) -> bool:
    _, (x1, y1, x2, y2) = bbox
    return blur_of_size(crop_ref.bbox_to_center_size(x1, y1, x2, y2, bbox_shape)[2], image_size) is not None
