"""The numpy statement of hm_mask_boxes (include/hamer_hip.h, "Mask boxes"): per query ``np.where`` and four min / max.

``boxes(mask, queries)``: mask (N, H, W) uint8, queries a sequence of (frame, label) -> (Q, 5) int32 rows x1, y1, x2, y2, count.
A pixel belongs to a query when mask == label, or mask != 0 when label == -1; no such pixel, or a frame outside 0..N-1, gives
-1, -1, -1, -1, 0."""
import numpy as np

EMPTY = (-1, -1, -1, -1, 0)


def box(frame: np.ndarray, label: int):
    rows, cols = np.where(frame != 0) if label == -1 else np.where(frame == label)
    if len(rows) == 0:
        return EMPTY
    return int(cols.min()), int(rows.min()), int(cols.max()), int(rows.max()), int(len(rows))


def boxes(mask: np.ndarray, queries) -> np.ndarray:
    mask = np.asarray(mask)
    assert mask.ndim == 3 and mask.dtype == np.uint8
    out = np.empty((len(queries), 5), np.int32)
    for q, (frame, label) in enumerate(queries):
        out[q] = box(mask[frame], int(label)) if 0 <= frame < mask.shape[0] else EMPTY
    return out
