"""Hand meshes drawn onto their frames on the GPU (reference: hamer/reconstruct.py project_and_draw / main, :50-178; the
pyrender look of infer.py get_mesh_renderer / image_fusion and utils/mesh_renderer.py approximated per face by the ``shaded``
style and per pixel by ``render_views``).  The drawing rule is stated in include/hamer_hip.h (hm_mesh_overlay) and DESIGN.md section 8.

* ``overlay_frames``: device frames + meshes -> device frames, one hm_mesh_overlay call.
* ``render_views``: meshes -> per view RGBA, depth and mesh-label maps resolved per pixel by a z-buffer (hm_mesh_render, DESIGN.md
  section 8.1; reference utils/mesh_renderer.py:243-320), optionally drawn over frames: what ``MeshRenderer``, ``get_image``,
  the ``smooth`` folder style and ``hand_maps_folder`` (``--hand-maps``: label mask, depth and hand index per frame) stand on.
* ``skeleton_frames``: device images + device keypoints -> the 21-joint hand skeletons drawn onto them, one hm_skeleton_overlay
  call; ``openpose_radii`` restates the reference's OpenPose thickness arithmetic on the host.
* ``render_folder``: the ``.npy`` records of a folder job -> one overlay image per frame with hands, a batched MANO forward per
  pass of equally sized frames, PIL encoding on a small thread pool."""
from __future__ import annotations

import ctypes as C
import glob
import os
from concurrent.futures import ThreadPoolExecutor
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import lib as L

COLOR_RIGHT = (0, 255, 0)          # BGR: reconstruct.py's default green
COLOR_LEFT = (0, 255, 0)
STYLES = {"flat": L.HM_STYLE_FLAT, "shaded": L.HM_STYLE_SHADED}
FRAMES_PER_PASS = 16               # frames per overlay call of the folder paths: host memory and the key buffer scale with it
PASSES_IN_FLIGHT = 2               # passes whose encoded files may still be pending before the next pass is decoded

_ws: Dict[tuple, list] = {}        # (device index, stream) -> [workspace tensor, bytes known to hold 0xFF from offset 0]


def _workspace(device: torch.device, stream: int, need: int, key_bytes: int) -> torch.Tensor:
    """One growing workspace per (device, stream): calls on one stream are ordered, so they may share it; calls on two streams
    never do.  Its first ``key_bytes`` bytes hold 0xFF on return (the key buffer's contract).  ``release_workspaces`` frees
    them."""
    key = (device.index if device.index is not None else torch.cuda.current_device(), stream)
    ent = _ws.get(key)
    if ent is None or ent[0].numel() < need:
        _ws.pop(key, None)
        ent = _ws[key] = [torch.full((need,), 255, dtype=torch.uint8, device=device), need]
    if ent[1] < key_bytes:                       # bytes past the last call's keys held its face records
        ent[0][ent[1]:key_bytes].fill_(255)
    ent[1] = key_bytes                           # the call keeps its keys clean and writes records after them
    return ent[0]


def release_workspaces() -> None:
    """Drop the cached overlay workspaces (N*H*W*8 bytes of keys each, ~265 MB for 16 frames of 1080p).  Safe with work
    still enqueued: each workspace was allocated on the stream that uses it, and the caching allocator hands a freed block
    out again only in that stream's order."""
    _ws.clear()


def _mesh_color(m: dict, color_right, color_left):
    if m.get("color") is not None:
        return tuple(int(c) for c in m["color"])
    return tuple(color_right if m.get("is_right", True) else color_left)


def _pack_meshes(meshes: Sequence[dict], dev: torch.device, N: int, color=None):
    """The mesh table of one call and its concatenated device arrays: (table, verts fp64 (V,3), faces int32 (F,3), V, F)."""
    table = (L.Mesh * max(len(meshes), 1))()
    verts, faces, v0, f0 = [], [], 0, 0
    checked = {}                                 # (id of a faces object, nv) -> its range is known good (one sync per object)
    for i, m in enumerate(meshes):
        v = torch.as_tensor(m["vertices"]).to(dev, torch.float64).reshape(-1, 3)
        f = torch.as_tensor(m["faces"]).to(dev, torch.int32).reshape(-1, 3)
        ck = (id(m["faces"]), v.shape[0])
        if f.numel() and ck not in checked and not m.get("faces_checked"):     # a caller that checked them itself says so
            if v.shape[0] == 0 or int(f.min()) < 0 or int(f.max()) >= v.shape[0]:
                raise ValueError(f"mesh {i}: face corner outside its {v.shape[0]} vertices")
            checked[ck] = m["faces"]
        if not 0 <= int(m["frame"]) < N:
            raise ValueError(f"mesh {i}: frame {m['frame']} outside the batch of {N}")
        t = table[i]
        t.frame, t.v0, t.nv, t.f0, t.nf = int(m["frame"]), v0, v.shape[0], f0, f.shape[0]
        if color is not None:
            t.color_bgr[:] = color(m)
        verts.append(v); faces.append(f); v0 += v.shape[0]; f0 += f.shape[0]
    vd = torch.cat(verts).contiguous() if verts else torch.zeros(0, 3, dtype=torch.float64, device=dev)
    fd = torch.cat(faces).contiguous() if faces else torch.zeros(0, 3, dtype=torch.int32, device=dev)
    return table, vd, fd, v0, f0


def overlay_frames(frames_dev: torch.Tensor, K, meshes: Sequence[dict], style: str = "flat", alpha: float = 0.6,
                   color_right=COLOR_RIGHT, color_left=COLOR_LEFT, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """frames_dev (N,H,W,3) uint8 BGR on the GPU; K (3,3) for every frame or (N,3,3); meshes: dicts with ``frame``,
    ``vertices`` (V,3) camera-frame, ``faces`` (F,3) 0-based into the mesh's own vertices, and ``is_right`` or ``color``
    (B, G, R).  Returns a new (N,H,W,3) uint8 device tensor (or fills ``out``).  Enqueued on the current stream."""
    if style not in STYLES:
        raise ValueError(f"style must be one of {sorted(STYLES)}, got {style!r}")
    if not (frames_dev.is_cuda and frames_dev.dtype == torch.uint8 and frames_dev.dim() == 4 and frames_dev.shape[3] == 3):
        raise ValueError("frames_dev must be a (N,H,W,3) uint8 GPU tensor")
    frames_dev = frames_dev.contiguous()
    dev = frames_dev.device
    N, H, W, _ = frames_dev.shape
    Kt = torch.as_tensor(np.asarray(K.cpu() if torch.is_tensor(K) else K, dtype=np.float64))
    Kt = Kt.expand(N, 3, 3) if Kt.dim() == 2 else Kt
    if tuple(Kt.shape) != (N, 3, 3):
        raise ValueError(f"K must be (3,3) or ({N},3,3), got {tuple(Kt.shape)}")
    Kd = Kt.contiguous().to(dev)
    table, vd, fd, v0, f0 = _pack_meshes(meshes, dev, N, lambda m: _mesh_color(m, color_right, color_left))
    if out is None:
        out = torch.empty_like(frames_dev)
    elif not (out.device == dev and out.dtype == torch.uint8 and tuple(out.shape) == tuple(frames_dev.shape) and out.is_contiguous()):
        raise ValueError(f"out must be a contiguous uint8 tensor of shape {tuple(frames_dev.shape)} on {dev}")
    lib = L.load()
    need = lib.hm_mesh_overlay_workspace_bytes(N, H, W, len(meshes), f0)
    with torch.cuda.device(dev):
        ws = _workspace(dev, L.current_stream(), need, N * H * W * 8)
        L.check(lib.hm_mesh_overlay(L.ptr(frames_dev), N, H, W, L.ptr(Kd), L.ptr(vd) if v0 else None, v0,
                                    L.ptr(fd) if f0 else None, f0, table, len(meshes), STYLES[style], float(alpha), L.ptr(out),
                                    L.ptr(ws), ws.numel(), L.current_stream()), "hm_mesh_overlay")
    return out


RENDER_OUTPUTS = ("rgba", "depth", "mesh_id")
BASE_COLOR = (1.0, 1.0, 0.9)       # MeshRenderer's default baseColorFactor, R G B


def render_views(H: int, W: int, K, meshes: Sequence[dict], *, frames: Optional[torch.Tensor] = None,
                 outputs: Sequence[str] = RENDER_OUTPUTS, base_color=BASE_COLOR, bg=(0, 0, 0, 0), znear: float = 0.05,
                 views: Optional[int] = None, device=None) -> Dict[str, torch.Tensor]:
    """The z-buffered renderer (hm_mesh_render; the rule is in include/hamer_hip.h and DESIGN.md section 8.1): N views of
    H x W pixels, every mesh drawn into the view its ``frame`` names (the meshes format of ``overlay_frames``; colours are not
    used).  K (3,3) for every view or (N,3,3), last row exactly (0, 0, 1).  Returns a dict of new device tensors, one per name
    in ``outputs``: ``rgba`` (N,H,W,4) uint8 R G B A (uncovered: ``bg``), ``depth`` (N,H,W) float32 (uncovered 0),
    ``mesh_id`` (N,H,W) int32, a mesh's position in ``meshes`` (uncovered -1); with ``frames`` (N,H,W,3) uint8 BGR on the
    GPU also ``out``, the frames with the colour drawn over them.  N is ``views``, else the frames', else K's, else one more
    than the largest ``frame``.  One call, enqueued on the current stream; the workspace is the overlay's (per device and
    stream, ``release_workspaces``)."""
    unknown = [o for o in outputs if o not in RENDER_OUTPUTS]
    if unknown:
        raise ValueError(f"outputs must be among {RENDER_OUTPUTS}, got {unknown}")
    Kh = np.asarray(K.cpu() if torch.is_tensor(K) else K, dtype=np.float64)
    if frames is not None:
        if not (frames.is_cuda and frames.dtype == torch.uint8 and frames.dim() == 4 and frames.shape[3] == 3
                and tuple(frames.shape[1:3]) == (H, W)):
            raise ValueError(f"frames must be a (N,{H},{W},3) uint8 GPU tensor")
        frames = frames.contiguous()
    elif not outputs:
        raise ValueError("no output requested")
    N = views if views is not None else frames.shape[0] if frames is not None else Kh.shape[0] if Kh.ndim == 3 else \
        max([int(m["frame"]) for m in meshes], default=0) + 1
    if frames is not None and frames.shape[0] != N:
        raise ValueError(f"{frames.shape[0]} frames for {N} views")
    Kh = np.broadcast_to(Kh, (N, 3, 3)) if Kh.ndim == 2 else Kh
    if tuple(Kh.shape) != (N, 3, 3):
        raise ValueError(f"K must be (3,3) or ({N},3,3), got {tuple(Kh.shape)}")
    Kh = np.ascontiguousarray(Kh)
    if device is not None:
        dev = torch.device(device)
    elif frames is not None:
        dev = frames.device
    else:
        dev = next((m["vertices"].device for m in meshes if torch.is_tensor(m["vertices"]) and m["vertices"].is_cuda),
                   torch.device("cuda", torch.cuda.current_device()))
    table, vd, fd, v0, f0 = _pack_meshes(meshes, dev, N)
    res = {}
    if "rgba" in outputs:
        res["rgba"] = torch.empty(N, H, W, 4, dtype=torch.uint8, device=dev)
    if "depth" in outputs:
        res["depth"] = torch.empty(N, H, W, dtype=torch.float32, device=dev)
    if "mesh_id" in outputs:
        res["mesh_id"] = torch.empty(N, H, W, dtype=torch.int32, device=dev)
    if frames is not None:
        res["out"] = torch.empty_like(frames)
    base = (C.c_double * 3)(*[float(c) for c in base_color])
    bgc = (C.c_uint8 * 4)(*[int(c) for c in bg])
    lib = L.load()
    need = lib.hm_mesh_render_workspace_bytes(N, H, W, v0, len(meshes), f0)
    with torch.cuda.device(dev):
        ws = _workspace(dev, L.current_stream(), need, N * H * W * 8)
        L.check(lib.hm_mesh_render(N, H, W, Kh.ctypes.data_as(C.POINTER(C.c_double)), L.ptr(vd) if v0 else None, v0,
                                   L.ptr(fd) if f0 else None, f0, table, len(meshes), base, bgc, float(znear), L.ptr(frames),
                                   L.ptr(res.get("out")), L.ptr(res.get("rgba")), L.ptr(res.get("depth")),
                                   L.ptr(res.get("mesh_id")), L.ptr(ws), ws.numel(), L.current_stream()), "hm_mesh_render")
    return res


# ------------------------------------------------------------------------------------------------ hand skeletons (section 8.2)
# hamer/utils/draw_2d_skeleton.py:9-14 (0..1; its index finger differs from vis_tool's COLOR_HAND_JOINTS)
COLOR_HAND_JOINTS_HAMER = [[1.0, 0.0, 0.0],
                           [0.0, 0.4, 0.0], [0.0, 0.6, 0.0], [0.0, 0.8, 0.0], [0.0, 1.0, 0.0],
                           [0.0, 0.0, 0.4], [0.0, 0.0, 0.6], [0.0, 0.0, 0.8], [0.0, 0.0, 1.0],
                           [0.0, 0.4, 0.4], [0.0, 0.6, 0.6], [0.0, 0.8, 0.8], [0.0, 1.0, 1.0],
                           [0.4, 0.4, 0.0], [0.6, 0.6, 0.0], [0.8, 0.8, 0.0], [1.0, 1.0, 0.0],
                           [0.4, 0.0, 0.4], [0.6, 0.0, 0.6], [0.8, 0.0, 0.8], [1.0, 0.0, 1.0]]
# hamer/utils/render_openpose.py:105-125 (0..255)
COLOR_OPENPOSE_HAND = [[100, 100, 100],
                       [100, 0, 0], [150, 0, 0], [200, 0, 0], [255, 0, 0],
                       [100, 100, 0], [150, 150, 0], [200, 200, 0], [255, 255, 0],
                       [0, 100, 50], [0, 150, 75], [0, 200, 100], [0, 255, 125],
                       [0, 50, 100], [0, 75, 150], [0, 100, 200], [0, 125, 255],
                       [100, 0, 100], [150, 0, 150], [200, 0, 200], [255, 0, 255]]
# style -> (order, default line_radius, default joint_radius).  'sar': vis_tool's line width 1 / radius 2 (the host rule of
# rootnet/Model_RGB.py draw_2d_skeleton); 'hamer': draw_2d_skeleton.py's line_wd 2 / marker_sz 3; 'openpose': openpose_radii
SKELETON_STYLES = {"sar": (L.HM_SKEL_INTERLEAVED, 0, 2), "hamer": (L.HM_SKEL_INTERLEAVED, 1, 3),
                   "openpose": (L.HM_SKEL_BONES_FIRST, None, None)}


def skeleton_palette(style: str) -> np.ndarray:
    """(21, 3) uint8: colour j of bone j and joint j, its bytes going to channels 0, 1, 2 of the image as it is stored."""
    if style == "sar":
        from .rootnet.Model_RGB import COLOR_HAND_JOINTS
        return np.round(np.array(COLOR_HAND_JOINTS) * 255).astype(np.uint8)
    if style == "hamer":
        return np.round(np.array(COLOR_HAND_JOINTS_HAMER) * 255).astype(np.uint8)
    if style == "openpose":
        return np.array(COLOR_OPENPOSE_HAND, np.uint8)
    raise ValueError(f"style must be one of {sorted(SKELETON_STYLES)}, got {style!r}")


def openpose_radii(H: int, W: int, keypoints_host) -> Optional[tuple]:
    """(line_radius, joint_radius) of one hand drawn as render_hand_keypoints does, or None when it draws nothing.
    Restates render_keypoints (render_openpose.py:56-71) with thickness_circle_ratio 1/50, line ratio 0.75, pose scale 1 and
    the rectangle threshold 0.1 -- including its quirk: ``width, height = img.shape[1], img.shape[2]``, so the "height" is
    the channel count 3 whatever ``H`` is.  keypoints_host (21, 2 | 3): without a confidence column every joint counts.
    cv2 then draws rings ``circle(radius R, thickness T)`` and lines of thickness T; OUR mapping to the rule's filled
    primitives is joint_radius = R + T // 2 (the ring's outer edge) and line_radius = T // 2."""
    kp = np.asarray(keypoints_host)
    kp = (kp if kp.dtype.kind == "f" else kp.astype(np.float64)).reshape(21, -1)
    valid = kp[:, 2] > 0.1 if kp.shape[1] >= 3 else np.ones(21, bool)        # compared in the keypoints' own precision
    if not valid.any():
        return None
    xy = kp[valid, :2].astype(np.float64)
    pw, ph = xy[:, 0].max() - xy[:, 0].min(), xy[:, 1].max() - xy[:, 1].min()
    if not pw * ph > 0:
        return None
    width, height = float(W), 3.0
    ratio = min(1.0, max(pw / width, ph / height))
    thickness_ratio = max(np.round(np.sqrt(width * height) * (1.0 / 50) * ratio), 2.0)
    thickness_circle = max(1.0, thickness_ratio if ratio > 0.05 else -1.0)
    thickness_line = max(1.0, np.round(thickness_ratio * 0.75))
    R, Tc, Tl = int(round(thickness_ratio / 2)), int(round(thickness_circle)), int(round(thickness_line))
    return Tl // 2, R + Tc // 2


def _per_hand(value, default, n: int, what: str) -> List[int]:
    if value is None:
        value = default
    if value is None:
        raise ValueError(f"style 'openpose' takes its {what} from openpose_radii(H, W, keypoints on the host): pass {what} "
                         "(one int or one per hand), or host keypoints")
    v = [int(value)] * n if np.ndim(value) == 0 else [int(x) for x in value]
    if len(v) != n:
        raise ValueError(f"{what}: {len(v)} values for {n} hands")
    if any(not 0 <= x <= 32 for x in v):
        raise ValueError(f"{what} must be in 0..32, got {value}")
    return v


def skeleton_frames(images_dev: torch.Tensor, keypoints, image_index: Sequence[int], style: str = "hamer", line_radius=None,
                    joint_radius=None, threshold: float = 0.1, out: Optional[torch.Tensor] = None,
                    inplace: bool = False) -> torch.Tensor:
    """Draw hand skeletons (hm_skeleton_overlay; the rule is in include/hamer_hip.h and DESIGN.md section 8.2).  images_dev
    (N,H,W,3) uint8 on the GPU; keypoints (n,21,2) pixels or (n,21,3) with a confidence (a joint is drawn if conf >
    ``threshold``), a device tensor (never read back) or a host array; image_index: per hand the image it is drawn into, in
    drawing order (a later hand goes over an earlier one).  Non-finite or out-of-range joints are left out with their bones.
    style: 'sar' (vis_tool's colours), 'hamer' (draw_2d_skeleton.py's), 'openpose' (render_openpose.py's, bones first);
    colours go to channels 0, 1, 2 as the image stores them.  line_radius / joint_radius: one int or one per hand, default by
    style; for 'openpose' the default is ``openpose_radii`` per hand, which needs HOST keypoints (hands it would not draw are
    left out).  Returns a new tensor, or ``out``, or with ``inplace`` images_dev itself (only the hands' boxes are touched).
    One call, enqueued on the current stream, no synchronisation."""
    if style not in SKELETON_STYLES:
        raise ValueError(f"style must be one of {sorted(SKELETON_STYLES)}, got {style!r}")
    if not (torch.is_tensor(images_dev) and images_dev.is_cuda and images_dev.dtype == torch.uint8 and images_dev.dim() == 4
            and images_dev.shape[3] == 3):
        raise ValueError("images_dev must be a (N,H,W,3) uint8 GPU tensor")
    if inplace and not images_dev.is_contiguous():
        raise ValueError("inplace needs contiguous images")
    if inplace and out is not None:
        raise ValueError("give out or inplace, not both")
    images_dev = images_dev.contiguous()
    dev = images_dev.device
    N, H, W, _ = images_dev.shape
    order, d_line, d_joint = SKELETON_STYLES[style]
    image_index = [int(i) for i in image_index]
    n = len(image_index)
    host_kp = None if torch.is_tensor(keypoints) and keypoints.is_cuda else np.asarray(
        keypoints.cpu() if torch.is_tensor(keypoints) else keypoints, np.float32)
    if style == "openpose" and host_kp is not None and n and (line_radius is None or joint_radius is None):
        radii = [openpose_radii(H, W, k) for k in host_kp.reshape(n, 21, -1)]
        keep = [i for i, r in enumerate(radii) if r is not None]
        if line_radius is None:
            line_radius = [radii[i][0] for i in keep]
        elif np.ndim(line_radius):
            line_radius = [line_radius[i] for i in keep]
        if joint_radius is None:
            joint_radius = [radii[i][1] for i in keep]
        elif np.ndim(joint_radius):
            joint_radius = [joint_radius[i] for i in keep]
        host_kp, image_index, n = host_kp.reshape(n, 21, -1)[keep], [image_index[i] for i in keep], len(keep)
    kd = (torch.from_numpy(np.ascontiguousarray(host_kp)).to(dev) if host_kp is not None else keypoints.to(dev)).to(torch.float32)
    if n and (kd.dim() != 3 or kd.shape[0] != n or kd.shape[1] != 21 or kd.shape[2] not in (2, 3)):
        raise ValueError(f"keypoints must be ({n},21,2) or ({n},21,3), got {tuple(kd.shape)}")
    kd = kd.contiguous()
    lr, jr = _per_hand(line_radius, d_line, n, "line_radius"), _per_hand(joint_radius, d_joint, n, "joint_radius")
    table = (L.Skeleton * max(n, 1))()
    for i in range(n):
        if not 0 <= image_index[i] < N:
            raise ValueError(f"hand {i}: image {image_index[i]} outside the batch of {N}")
        table[i].image, table[i].line_radius, table[i].joint_radius, table[i].threshold = image_index[i], lr[i], jr[i], float(threshold)
    if inplace:
        out = images_dev
    elif out is None:
        out = torch.empty_like(images_dev)
    elif not (out.device == dev and out.dtype == torch.uint8 and tuple(out.shape) == tuple(images_dev.shape) and out.is_contiguous()):
        raise ValueError(f"out must be a contiguous uint8 tensor of shape {tuple(images_dev.shape)} on {dev}")
    pal = np.ascontiguousarray(skeleton_palette(style))
    lib = L.load()
    need = lib.hm_skeleton_overlay_workspace_bytes(N, H, W, n)
    with torch.cuda.device(dev):
        ws = torch.empty(max(need, 8), dtype=torch.uint8, device=dev)      # the call zeroes what it reads; freed in stream order
        L.check(lib.hm_skeleton_overlay(L.ptr(images_dev), N, H, W, L.ptr(kd) if n else None, int(kd.shape[2]) if n else 2,
                                        table, n, pal.ctypes.data_as(C.POINTER(C.c_uint8)), order, L.ptr(out), L.ptr(ws),
                                        ws.numel(), L.current_stream()), "hm_skeleton_overlay")
    return out


def default_camera(H: int, W: int, cfg) -> np.ndarray:
    """The camera the records were made with when no intrinsics are given (infer.py _estimate, no-intrinsics branch):
    fx = fy = EXTRA.FOCAL_LENGTH / MODEL.IMAGE_SIZE * max(H, W), principal point at the frame centre."""
    f = float(cfg.EXTRA.FOCAL_LENGTH) / float(cfg.MODEL.IMAGE_SIZE) * max(H, W)
    return np.array([[f, 0.0, W / 2.0], [0.0, f, H / 2.0], [0.0, 0.0, 1.0]], np.float64)


def camera_vertices(hamer, hands: List[dict]) -> torch.Tensor:
    """(B, V, 3) fp32 camera-frame vertices of the hand records: MANO (one forward), x := -x for left hands, += cam_t --
    the vertices of the OBJ reconstruct_and_save_obj_with_wrapper writes, before its ``%.8f`` text."""
    from .infer import mano_hand_vertices
    dev = hamer.device
    verts = mano_hand_vertices(hamer, hands)
    sign = torch.tensor([[1.0, 1.0, 1.0] if h["is_right"] else [-1.0, 1.0, 1.0] for h in hands], device=dev)
    cam_t = torch.tensor(np.stack([np.asarray(h["cam_t"], np.float32).reshape(3) for h in hands]), device=dev)
    return verts * sign[:, None, :] + cam_t[:, None, :]


def camera_joints_vertices(hamer, hands: List[dict]):
    """``camera_vertices`` with the 21 MANO joints placed the same way: (joints (B, 21, 3), vertices (B, V, 3)) fp32 in the
    camera frame, from one MANO forward."""
    from .infer import mano_hand_joints_vertices
    dev = hamer.device
    joints, verts = mano_hand_joints_vertices(hamer, hands)
    sign = torch.tensor([[1.0, 1.0, 1.0] if h["is_right"] else [-1.0, 1.0, 1.0] for h in hands], device=dev)
    cam_t = torch.tensor(np.stack([np.asarray(h["cam_t"], np.float32).reshape(3) for h in hands]), device=dev)
    return joints * sign[:, None, :] + cam_t[:, None, :], verts * sign[:, None, :] + cam_t[:, None, :]


def project_points(points: torch.Tensor, K) -> torch.Tensor:
    """Camera-frame points (..., 3) on the device -> pixels (..., 2) fp32 by section 8's rule, in fp64 with plain torch ops
    (one rounding each, left to right): z == 0 -> 1e-5, w = K20*x + K21*y + K22*z, u = (K00*x + K01*y + K02*z) / w,
    v = (K10*x + K11*y + K12*z) / w, rounded once to fp32.  Points with z <= 0 become NaN (the skeleton rule leaves them out)."""
    k = np.asarray(K.cpu() if torch.is_tensor(K) else K, np.float64)
    p = points.to(torch.float64)
    x, y, z0 = p[..., 0], p[..., 1], p[..., 2]
    z = torch.where(z0 == 0.0, torch.full_like(z0, 1e-5), z0)
    w = float(k[2, 0]) * x + float(k[2, 1]) * y + float(k[2, 2]) * z
    u = (float(k[0, 0]) * x + float(k[0, 1]) * y + float(k[0, 2]) * z) / w
    v = (float(k[1, 0]) * x + float(k[1, 1]) * y + float(k[1, 2]) * z) / w
    uv = torch.stack([u, v], dim=-1)
    return torch.where((z0 > 0.0)[..., None], uv, torch.full_like(uv, float("nan"))).to(torch.float32)


def _encode_threads() -> int:
    try:
        n = len(os.sched_getaffinity(0))
    except AttributeError:
        n = os.cpu_count() or 1
    return max(1, min(16, n))


def _save(path: str, img_bgr: np.ndarray) -> None:
    from PIL import Image
    Image.fromarray(np.ascontiguousarray(img_bgr[:, :, ::-1])).save(path)


def frame_size(path: str) -> Optional[tuple]:
    """(H, W) of an image from its header (PIL opens lazily: no pixel is decoded); None when unreadable."""
    try:
        from PIL import Image
        with Image.open(path) as im:
            w, h = im.size
        return h, w
    except Exception:
        return None


def size_passes(sizes: Sequence[Optional[tuple]], per_pass: int) -> List[tuple]:
    """[(size, [indices])] -- the items grouped by frame size (first-seen order, input order inside a group) and cut into
    passes of at most ``per_pass``; items of size None are left out."""
    groups: Dict[tuple, List[int]] = {}
    for i, hw in enumerate(sizes):
        if hw is not None:
            groups.setdefault(tuple(hw), []).append(i)
    return [(hw, idx[s:s + per_pass]) for hw, idx in groups.items() for s in range(0, len(idx), per_pass)]


class PassWriter:
    """Encodes a pass's images on ``pool`` and keeps at most ``in_flight`` passes pending: submitting one more first waits
    for the oldest, so host memory holds a bounded number of decoded outputs however long the folder."""

    def __init__(self, pool, in_flight: int = PASSES_IN_FLIGHT, save=None):
        self.pool, self.in_flight, self.pending, self.written, self.save = pool, in_flight, [], 0, save or _save

    def _finish_oldest(self):
        for f in self.pending.pop(0):
            f.result()
            self.written += 1

    def submit(self, items) -> None:
        """items: (path, (H,W,3) uint8 BGR), or the arguments of the writer's own ``save``."""
        while len(self.pending) >= self.in_flight:
            self._finish_oldest()
        self.pending.append([self.pool.submit(self.save, *item) for item in items])

    def close(self) -> int:
        while self.pending:
            self._finish_oldest()
        return self.written


def decode_pass(pool, paths: Sequence[str], hw: tuple):
    """The frames of one pass as one (n, H, W, 3) uint8 array (decoded on ``pool``) and the indices that decoded to (H, W)."""
    from .infer import _imread_bgr
    frames = list(pool.map(_imread_bgr, paths))
    ok = [i for i, fr in enumerate(frames) if fr is not None and fr.shape[:2] == tuple(hw)]
    for i in sorted(set(range(len(paths))) - set(ok)):
        print(f"Skipping {paths[i]}: image load failed")
    return (np.stack([frames[i] for i in ok]) if ok else None), ok


def render_folder(image_folder, npy_folder, out_folder, hamer, k_real=None, style: str = "flat", rank: int = 0, world: int = 1,
                  ext: str = ".jpg", frames_per_pass: int = FRAMES_PER_PASS, keypoints: Optional[str] = None,
                  keypoint_style: str = "hamer", line_radius=None, joint_radius=None, visible_joints: bool = False) -> int:
    """Draw the hands of every ``<name>.npy`` record of ``npy_folder`` onto ``image_folder``'s ``<name>.*`` frame and write
    ``out_folder/<name><ext>`` (``.jpg`` as the reference; any extension PIL writes).  Frames are grouped by the size their
    headers give and drawn in passes of ``frames_per_pass``: per pass the frames are decoded, ONE MANO forward runs for all its
    hands (the formulation of reconstruct_and_save_obj_with_wrapper), one overlay call (``style`` "flat" or "shaded":
    ``overlay_frames``; "smooth": the z-buffered ``render_views``), one copy back, and the encodes go to
    a ``PassWriter`` -- host memory stays bounded by a few passes whatever the folder's length.  ``k_real`` None: the camera
    the records were made with (``default_camera``).  ``rank`` / ``world``: this process draws ``shard_paths(records, rank,
    world)``.  ``keypoints``: None, or 'over' / 'only' to draw the hands' 21 MANO joints as skeletons (``skeleton_frames``,
    ``keypoint_style`` and radii as there) over the mesh overlay / onto the decoded frames instead of it: the joints of the
    pass's MANO forward, mirrored and translated like the vertices, projected on the device (``project_points``), one call in
    place.  ``visible_joints`` (with ``keypoints``): a joint whose code in the record's ``joints_visible``
    (``evaluate_visibility.annotate_folder``) is not 0 is absent, and so are its bones -- through the
    skeleton rule's confidence column (1 or 0); a hand without ``joints_visible`` draws all its joints, which is said once.
    Returns the number of images written; the overlay workspaces are released at the end."""
    if keypoints not in (None, "over", "only"):
        raise ValueError(f"keypoints must be None, 'over' or 'only', got {keypoints!r}")
    if visible_joints and not keypoints:
        raise ValueError("visible_joints needs keypoints 'over' or 'only'")
    if keypoints and keypoint_style not in SKELETON_STYLES:
        raise ValueError(f"keypoint_style must be one of {sorted(SKELETON_STYLES)}, got {keypoint_style!r}")
    os.makedirs(out_folder, exist_ok=True)
    jobs = _record_jobs(image_folder, npy_folder, rank, world, keep_empty=False)
    dev = hamer.device
    faces = torch.as_tensor(np.asarray(hamer.mano.faces, np.int32), device=dev)
    try:
        with ThreadPoolExecutor(_encode_threads()) as pool:
            writer = PassWriter(pool)
            sizes = list(pool.map(frame_size, [j[1] for j in jobs]))
            for i in (i for i, hw in enumerate(sizes) if hw is None):
                print(f"Skipping {jobs[i][0]}: image load failed")
            for (H, W), part in size_passes(sizes, frames_per_pass):
                batch, ok = decode_pass(pool, [jobs[i][1] for i in part], (H, W))
                if batch is None:
                    continue
                part = [part[k] for k in ok]
                K = np.asarray(k_real, np.float64) if k_real is not None else default_camera(H, W, hamer.cfg)
                hands = [(n, h) for n, i in enumerate(part) for h in jobs[i][2]]
                if keypoints:
                    joints, verts = camera_joints_vertices(hamer, [h for _, h in hands])
                else:
                    verts = camera_vertices(hamer, [h for _, h in hands])
                meshes = [{"frame": n, "vertices": verts[j], "faces": faces, "is_right": bool(h["is_right"])}
                          for j, (n, h) in enumerate(hands)]
                if keypoints == "only":
                    out = torch.from_numpy(batch).to(dev)
                elif style == "smooth":
                    out = render_views(H, W, K, meshes, frames=torch.from_numpy(batch).to(dev), outputs=())["out"]
                else:
                    out = overlay_frames(torch.from_numpy(batch).to(dev), K, meshes, style=style)
                if keypoints:
                    kp = project_points(joints, K)
                    if visible_joints:
                        kp = torch.cat([kp, torch.from_numpy(joint_confidences([h for _, h in hands])).to(dev)[..., None]], dim=2)
                    if keypoint_style == "openpose" and (line_radius is None or joint_radius is None):
                        kp = kp.cpu().numpy()                          # the OpenPose thickness is host arithmetic on the keypoints
                    skeleton_frames(out, kp, [n for n, _ in hands], style=keypoint_style, line_radius=line_radius,
                                    joint_radius=joint_radius, inplace=True)
                res = out.cpu().numpy()
                writer.submit([(os.path.join(out_folder, jobs[i][0] + ext), res[n]) for n, i in enumerate(part)])
            return writer.close()
    finally:
        release_workspaces()


_said_no_flags = []


def joint_confidences(hands: Sequence[dict]) -> np.ndarray:
    """(n, 21) float32 for the skeleton rule's confidence column: 1 where a hand record's ``joints_visible`` code is 0
    (VISIBLE), 0 elsewhere; all 1 for a record without the key, with one printed line the first time."""
    conf = np.ones((len(hands), 21), np.float32)
    for j, h in enumerate(hands):
        flags = h.get("joints_visible")
        if flags is None:
            if not _said_no_flags:
                _said_no_flags.append(True)
                print("visible_joints: a record has no joints_visible (write it with --visibility or evaluate_visibility --write-to): all its joints are drawn")
            continue
        conf[j] = (np.asarray(flags).reshape(21) == 0).astype(np.float32)
    return conf


def _record_jobs(image_folder, npy_folder, rank: int, world: int, keep_empty: bool):
    """(stem, frame path, hand records in right, left order) of this rank's share of the records that have a frame."""
    from .infer import _list_images, shard_paths
    frames_by_stem = {os.path.splitext(os.path.basename(p))[0]: p for p in _list_images(image_folder)}
    jobs = []
    for npy in shard_paths(sorted(glob.glob(os.path.join(npy_folder, "*.npy"))), rank, world):
        stem = os.path.splitext(os.path.basename(npy))[0]
        if stem not in frames_by_stem:
            continue
        data = np.load(npy, allow_pickle=True).item()
        hands = [data[t] for t in ("right", "left") if data.get(t) is not None]
        if hands or keep_empty:
            jobs.append((stem, frames_by_stem[stem], hands))
    return jobs


def _save_maps(out_folder: str, stem: str, label: np.ndarray, depth: np.ndarray, hand: np.ndarray) -> None:
    np.save(os.path.join(out_folder, stem + ".npy"), label)
    np.savez_compressed(os.path.join(out_folder, stem + "_maps.npz"), depth=depth, hand=hand)


def hand_maps_folder(image_folder, npy_folder, out_folder, hamer, k_real=None, label: int = 3, rank: int = 0, world: int = 1,
                     frames_per_pass: int = FRAMES_PER_PASS) -> int:
    """Per ``<stem>.npy`` record of ``npy_folder`` with a frame in ``image_folder``: which pixels its hands cover, how far
    away, and which hand.  Writes ``out_folder/<stem>.npy``, uint8 (H, W) with ``label`` on hand pixels and 0 elsewhere -- the
    label mask get_bbox_from_npy / process_batch_manopara_with_mask read -- and ``<stem>_maps.npz`` with ``depth`` (float32
    metres, 0 = none) and ``hand`` (int8 index into the record's hands in right, left order, -1 = none).  The frame size comes
    from the image header (``frame_size``): no frame is decoded.  Streams in passes like ``render_folder``: one MANO forward
    and one ``render_views`` call per pass of equally sized frames.  A record without hands gets empty maps.  Returns the
    number of records written; the workspaces are released at the end."""
    if not 1 <= int(label) <= 255:
        raise ValueError(f"label must be in 1..255, got {label}")
    os.makedirs(out_folder, exist_ok=True)
    jobs = _record_jobs(image_folder, npy_folder, rank, world, keep_empty=True)
    dev = hamer.device
    faces = torch.as_tensor(np.asarray(hamer.mano.faces, np.int32), device=dev)
    try:
        with ThreadPoolExecutor(_encode_threads()) as pool:
            writer = PassWriter(pool, save=_save_maps)
            sizes = list(pool.map(frame_size, [j[1] for j in jobs]))
            for i in (i for i, hw in enumerate(sizes) if hw is None):
                print(f"Skipping {jobs[i][0]}: image load failed")
            for (H, W), part in size_passes(sizes, frames_per_pass):
                K = np.asarray(k_real, np.float64) if k_real is not None else default_camera(H, W, hamer.cfg)
                hands = [(n, h) for n, i in enumerate(part) for h in jobs[i][2]]
                first = np.cumsum([0] + [len(jobs[i][2]) for i in part])[:-1]      # a frame's first row of the mesh table
                meshes = []
                if hands:
                    verts = camera_vertices(hamer, [h for _, h in hands])
                    meshes = [{"frame": n, "vertices": verts[j], "faces": faces} for j, (n, _) in enumerate(hands)]
                r = render_views(H, W, K, meshes, outputs=("depth", "mesh_id"), views=len(part), device=dev)
                mid = r["mesh_id"]
                hand = torch.where(mid >= 0, mid - torch.as_tensor(first, dtype=torch.int32, device=dev)[:, None, None],
                                   mid).to(torch.int8)
                lab = ((mid >= 0).to(torch.uint8) * int(label)).cpu().numpy()
                depth, hand = r["depth"].cpu().numpy(), hand.cpu().numpy()
                writer.submit([(out_folder, jobs[i][0], lab[n], depth[n], hand[n]) for n, i in enumerate(part)])
            return writer.close()
    finally:
        release_workspaces()
