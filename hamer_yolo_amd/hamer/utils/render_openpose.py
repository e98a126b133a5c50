"""hamer/utils/render_openpose.py of the reference, hands only, drawn by one HIP call (hm_skeleton_overlay).

``get_keypoints_rectangle``, ``render_hand_keypoints`` and ``render_openpose`` keep the reference's signatures: numpy in,
numpy out.  The thickness arithmetic of ``render_keypoints`` (:56-71, with its ``img.shape[2]`` quirk) is restated by
``render.openpose_radii``; cv2's rings and thick lines become the filled discs and round-capped bones of DESIGN.md section 8.2
(joint_radius = R + T // 2, line_radius = T // 2), bones first, opaque.  Body keypoints, ``use_confidence`` thickness maps and
alpha blending are not served.  There is no CPU fallback."""
from __future__ import annotations

from typing import Tuple

import numpy as np
import torch

from ...render import skeleton_frames
from .draw_2d_skeleton import _device


def get_keypoints_rectangle(keypoints: np.ndarray, threshold: float) -> Tuple[float, float, float]:
    """Width, height and area of the rectangle around the keypoints (N, 3) whose confidence is above the threshold
    (render_openpose.py:10-31); (0, 0, 0) when there is none."""
    keypoints = np.asarray(keypoints)
    valid = keypoints[:, -1] > threshold
    if valid.sum() > 0:
        v = keypoints[valid][:, :-1]
        width, height = v[:, 0].max() - v[:, 0].min(), v[:, 1].max() - v[:, 1].min()
        return width, height, width * height
    return 0, 0, 0


def render_hand_keypoints(img, right_hand_keypoints, threshold=0.1, use_confidence=False, map_fn=None, alpha=1.0):
    """img (H, W, 3) with values in 0..255, right_hand_keypoints (21, 3): x, y, confidence -> the image with the hand drawn
    (joints and bones whose confidences are above ``threshold``).  A uint8 image comes back as uint8; any other dtype is
    rounded to uint8 for the drawing and cast back.  ``alpha`` is accepted and unused, as in the reference."""
    if use_confidence:
        raise NotImplementedError("render_hand_keypoints: use_confidence (a thickness per joint) is not served")
    src = np.asarray(img)
    u8 = src if src.dtype == np.uint8 else np.clip(np.rint(src), 0, 255).astype(np.uint8)
    kp = np.asarray(right_hand_keypoints, np.float32).reshape(1, 21, 3)
    dev = _device()
    out = skeleton_frames(torch.from_numpy(np.ascontiguousarray(u8)).to(dev)[None], kp, [0], style="openpose", threshold=threshold)
    return out[0].cpu().numpy().astype(src.dtype, copy=False)


def render_openpose(img: np.ndarray, hand_keypoints: np.ndarray) -> np.ndarray:
    """render_openpose.py:179-191: the hand keypoints (21, 3) in the OpenPose format drawn onto img."""
    return render_hand_keypoints(img, hand_keypoints)
