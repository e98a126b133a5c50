"""The detector's test-time augmentation, stated in numpy: Model.forward(x, augment=True) (yolo.py:589-605) around
scale_img (utils/torch_utils.py:247-257).  For a letterboxed network input x of h x w in [0, 1]:

    for s, flip in ((1, no), (0.83, left-right), (0.67, no)):
        xi = scale_img(x mirrored if flip, s, gs=32)        resize to (int(h*s), int(w*s)), pad right / bottom with 0.447
        yi = forward_once(xi)                               to (ceil(h*s/32)*32, ceil(w*s/32)*32)
        yi[..., :4] /= s;  yi[..., 0] = w - yi[..., 0] if flip
    pred = concatenate(yi) per image

The resize is F.interpolate(mode='bilinear', align_corners=False): per axis, source index max(0, (in/out)*(d+0.5)-0.5) in
fp32 (in/out and d+0.5 rounded, the multiply-subtract fused, as torch evaluates it), second tap clamped to in-1.  Here the
taps and weights are computed in fp32 exactly so and the four-tap combination in float64 (what the fp32 and 16-bit kernels
are measured against)."""
import math

import numpy as np

SCALES = (1.0, 0.83, 0.67)
FLIPS = (False, True, False)
GS = 32
PAD = 0.447
STRIDES = (8, 16, 32)


def sizes(h, w, ratio, gs=GS):
    """(resized h, resized w, padded h, padded w), in Python's doubles."""
    return int(h * ratio), int(w * ratio), math.ceil(h * ratio / gs) * gs, math.ceil(w * ratio / gs) * gs


def taps(sn, dn, pn, flip=False):
    """One axis: (tap0, tap1) int32 and (weight0, weight1) float32 for the pn padded outputs of a resize sn -> dn; outputs
    past dn are padding: taps -1, weights 0.  ``flip``: taps into the unmirrored image."""
    f32 = np.float32
    i0, i1 = np.full(pn, -1, np.int32), np.full(pn, -1, np.int32)
    l0, l1 = np.zeros(pn, f32), np.zeros(pn, f32)
    scale = f32(sn) / f32(dn)
    d = np.arange(dn, dtype=f32)
    # scale * (d + 0.5) - 0.5 with ONE rounding (a fused multiply-add, as torch's kernels are compiled): the product of two
    # fp32 numbers and the difference are exact in float64 at these magnitudes, so the cast is that one rounding
    src = np.maximum((np.float64(scale) * (d + f32(0.5)).astype(np.float64) - 0.5).astype(f32), f32(0))
    assert src.dtype == f32
    a = src.astype(np.int32)
    b = a + (a < sn - 1)
    w1 = np.clip(src - a.astype(f32), f32(0), f32(1)).astype(f32)
    l0[:dn], l1[:dn] = f32(1) - w1, w1
    i0[:dn], i1[:dn] = (sn - 1 - a, sn - 1 - b) if flip else (a, b)
    return i0, i1, l0, l1


def table(h, w, ratio, gs=GS, flip=False):
    """The library's table layout: columns tap0 | tap1 | weight0 | weight1 (fp32 bits), then the rows; int32."""
    sh, sw, hp, wp = sizes(h, w, ratio, gs)
    parts = []
    for sn, dn, pn, fl in ((w, sw, wp, flip), (h, sh, hp, False)):
        i0, i1, l0, l1 = taps(sn, dn, pn, fl)
        parts += [i0, i1, l0.view(np.int32), l1.view(np.int32)]
    return np.concatenate(parts)


def scale_img(x, ratio, gs=GS, flip=False):
    """x (..., h, w) -> float64 (..., hp, wp): scale_img of x (mirrored left-right first when ``flip``)."""
    h, w = x.shape[-2:]
    sh, sw, hp, wp = sizes(h, w, ratio, gs)
    x0, x1, lx0, lx1 = taps(w, sw, wp, flip)
    y0, y1, ly0, ly1 = taps(h, sh, hp)
    xd = x.astype(np.float64)
    cols = xd[..., :, x0[:sw]] * lx0[:sw].astype(np.float64) + xd[..., :, x1[:sw]] * lx1[:sw].astype(np.float64)
    body = cols[..., y0[:sh], :] * ly0[:sh, None].astype(np.float64) + cols[..., y1[:sh], :] * ly1[:sh, None].astype(np.float64)
    out = np.full(x.shape[:-2] + (hp, wp), PAD, np.float64)
    out[..., :sh, :sw] = body
    return out


def level_rows(h, w):
    """rows of a prediction for an h x w network input: 3 anchors per cell of every level."""
    return [3 * (h // s) * (w // s) for s in STRIDES]


def n_rows(h, w):
    """rows per scale and in all for an h x w letterboxed input."""
    per = [sum(level_rows(*sizes(h, w, s)[2:])) for s in SCALES]
    return per, sum(per)


def descale(pred, ratio, flip, full_w):
    """yi[..., :4] /= s; yi[..., 0] = w - yi[..., 0] on an fp32 (.., 5+nc) array, as torch does on an fp32 tensor."""
    out = np.array(pred, dtype=np.float32, copy=True)
    out[..., :4] = out[..., :4] / np.float32(ratio)
    if flip:
        out[..., 0] = np.float32(full_w) - out[..., 0]
    return out


def torch_scale_img(img, ratio, gs=GS):
    """utils/torch_utils.py:247-257 (same_shape=False) restated on a (B, 3, h, w) torch tensor: the oracle's resize."""
    import torch.nn.functional as F
    if ratio == 1.0:
        return img
    h, w = img.shape[2:]
    s = (int(h * ratio), int(w * ratio))
    img = F.interpolate(img, size=s, mode='bilinear', align_corners=False)
    h, w = [math.ceil(x * ratio / gs) * gs for x in (h, w)]
    return F.pad(img, [0, w - s[1], 0, h - s[0]], value=PAD)


def oracle_pred(forward_once, x):
    """Model.forward(x, augment=True) (yolo.py:589-605) around ``forward_once(xi) -> (B, n, 5+nc)`` on a (B, 3, h, w) torch
    tensor: (pred (B, sum n, 5+nc), rows per scale)."""
    import torch
    w = x.shape[3]
    ys = []
    for s, flip in zip(SCALES, FLIPS):
        yi = forward_once(torch_scale_img(x.flip(3) if flip else x, s)).clone()
        yi[..., :4] /= s
        if flip:
            yi[..., 0] = w - yi[..., 0]
        ys.append(yi)
    return torch.cat(ys, 1), [y.shape[1] for y in ys]
