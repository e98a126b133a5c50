"""``MeshRenderer`` on the GPU (reference: hamer/hamer/utils/mesh_renderer.py:243-320, built by infer.py get_mesh_renderer,
:148-152): the reference's call signature over the z-buffered renderer of ``render.render_views`` (hm_mesh_render; the rule
is in include/hamer_hip.h and DESIGN.md section 8.1).  No pyrender, trimesh or OpenGL context: the lighting is the rule's
ambient + headlight term, smooth and two-sided, not pyrender's BRDF."""
from __future__ import annotations

import math

import numpy as np
import torch

BASE_COLOR_FACTOR = (1.0, 1.0, 0.9, 1.0)


def side_view_matrix(rot_angle: float = 90.0) -> np.ndarray:
    """The rotation by ``rot_angle`` degrees about the y axis through the origin (trimesh's
    ``rotation_matrix(radians(a), [0, 1, 0])``), (3,3) fp64; a vertex v becomes ``R @ v``."""
    a = math.radians(float(rot_angle))
    c, s = math.cos(a), math.sin(a)
    return np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]], np.float64)


def placed_vertices(vertices: torch.Tensor, cam_t: torch.Tensor, side_view: bool = False, rot_angle: float = 90.0) -> torch.Tensor:
    """(B,V,3) vertices and (B,3) translations -> fp64 camera-frame vertices: the side-view rotation first (about the origin of
    the vertices), then ``+ cam_t``."""
    v = vertices.to(torch.float64)
    if side_view:
        v = v @ torch.as_tensor(side_view_matrix(rot_angle), device=v.device).T
    return v + cam_t.to(v.device, torch.float64)[:, None, :]


class MeshRenderer:
    def __init__(self, cfg, faces):
        """``cfg``: the model config (EXTRA.FOCAL_LENGTH, MODEL.IMAGE_SIZE); ``faces``: (F,3) triangles of the hand mesh.
        Holds host data only: no device work happens before the first call."""
        if faces is None:
            raise TypeError("MeshRenderer needs the mesh's faces (F,3)")
        self.cfg = cfg
        self.focal_length = cfg.EXTRA.FOCAL_LENGTH
        self.img_res = cfg.MODEL.IMAGE_SIZE
        self.camera_center = [self.img_res // 2, self.img_res // 2]
        self.faces = np.ascontiguousarray(np.asarray(faces.cpu() if torch.is_tensor(faces) else faces, dtype=np.int32).reshape(-1, 3))
        self._faces_dev = {}

    def _faces_on(self, dev: torch.device) -> torch.Tensor:
        if dev not in self._faces_dev:
            self._faces_dev[dev] = torch.from_numpy(self.faces).to(dev)
        return self._faces_dev[dev]

    def render_hands(self, vertices, cam_t, H: int, W: int, focal, side_view: bool = False, rot_angle: float = 90.0,
                     base_color=BASE_COLOR_FACTOR[:3], outputs=("rgba",)):
        """B hands, each alone in a view of its own, in ONE render call: vertices (B,V,3), cam_t (B,3), focal a number or B
        numbers (fx = fy, principal point at the image centre).  Returns ``render_views``'s dict of device tensors with B
        views (``rgba`` (B,H,W,4) uint8 by default)."""
        from ... import render
        vertices = torch.as_tensor(vertices)
        if not vertices.is_cuda:
            vertices = vertices.cuda()
        if vertices.dim() == 2:
            vertices = vertices[None]
        B = vertices.shape[0]
        cam_t = torch.as_tensor(cam_t).reshape(B, 3)
        f = np.asarray(focal.detach().cpu() if torch.is_tensor(focal) else focal, np.float64).reshape(-1)
        f = np.broadcast_to(f[:1] if len(f) != B else f, (B,))
        K = np.zeros((B, 3, 3), np.float64)
        K[:, 0, 0] = K[:, 1, 1] = f
        K[:, 0, 2], K[:, 1, 2], K[:, 2, 2] = W / 2.0, H / 2.0, 1.0
        v = placed_vertices(vertices, cam_t, side_view, rot_angle)
        faces = self._faces_on(v.device)
        meshes = [{"frame": b, "vertices": v[b], "faces": faces} for b in range(B)]
        return render.render_views(H, W, K, meshes, outputs=outputs, base_color=base_color, views=B, device=v.device)

    def __call__(self, vertices, camera_translation, image, focal_length=5000, text=None, resize=None, side_view=False,
                 baseColorFactor=(1.0, 1.0, 0.9, 1.0), rot_angle=90, trans=None, do_flip=None, inv_trans=None):
        """The reference's signature.  vertices (V,3), camera_translation (3,), image: only its (H, W) is used.  Returns
        (H, W, 4) float32 RGBA in [0, 1] (bytes / 255; alpha 0 where no face covers the pixel).  fx = fy = ``focal_length``
        (a number or a tensor whose first element is taken), principal point at the image centre.  ``side_view`` rotates the
        vertices by ``rot_angle`` degrees about the y axis through the origin, before the translation.  The mesh stands at
        ``v + camera_translation``, where the OBJ and ``--render`` put it.  The reference's class passes the translation as
        the pyrender CAMERA pose and has dropped the x flip that used to go with it (:258-260), which mirrors ``tx``; that
        is not reproduced.  ``text``, ``resize``, ``trans``, ``do_flip`` and ``inv_trans`` are accepted and, as in the
        reference, have no effect."""
        H, W = int(image.shape[0]), int(image.shape[1])
        f = float(focal_length.flatten()[0]) if torch.is_tensor(focal_length) else float(focal_length)
        r = self.render_hands(torch.as_tensor(vertices)[None], torch.as_tensor(camera_translation).reshape(1, 3), H, W, f,
                              side_view=side_view, rot_angle=rot_angle, base_color=tuple(baseColorFactor)[:3])
        return r["rgba"][0].cpu().numpy().astype(np.float32) / 255.0
