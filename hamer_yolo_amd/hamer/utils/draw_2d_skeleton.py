"""hamer/utils/draw_2d_skeleton.py of the reference, drawn by one HIP call (hm_skeleton_overlay, csrc/skeleton.hip).

``draw_2d_skeleton(image, pose_uv)``: numpy in, numpy out, the reference's colours, topology and sizes (``line_wd`` 2 ->
line_radius 1, ``marker_sz`` 3 -> joint_radius 3) by the rule of DESIGN.md section 8.2.  The pixels are exact to that rule, not
to cv2.line / cv2.circle, and the reference's LINE_AA is not reproduced.  There is no CPU fallback."""
from __future__ import annotations

import numpy as np
import torch

from ...render import COLOR_HAND_JOINTS_HAMER as color_hand_joints  # noqa: F401  (the reference's module-level name)
from ...render import skeleton_frames


def _device() -> torch.device:
    from ... import lib as L
    L.load()                                            # HipLibraryError when the library is missing
    if not torch.cuda.is_available():
        raise L.HipLibraryError("hm_skeleton_overlay needs a GPU; there is no CPU path")
    return torch.device("cuda", torch.cuda.current_device())


def draw_2d_skeleton(image: np.ndarray, pose_uv: np.ndarray) -> np.ndarray:
    """image (H, W, 3) uint8, pose_uv (21, 2) pixels (wrist, then thumb .. little, four joints each) -> a new image with the
    skeleton drawn; colour bytes go to channels 0, 1, 2 as the image stores them, as the reference's do."""
    pose_uv = np.asarray(pose_uv)
    assert pose_uv.shape[0] == 21
    img = torch.from_numpy(np.ascontiguousarray(image, dtype=np.uint8)).to(_device())
    out = skeleton_frames(img[None], np.asarray(pose_uv[None, :, :2], np.float32), [0], style="hamer")
    return out[0].cpu().numpy()
