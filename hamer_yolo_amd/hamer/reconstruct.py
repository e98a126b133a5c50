"""The numeric half of the reference's reprojection check (reference: hamer/reconstruct.py:27-77): read the OBJ
written by ``reconstruct_and_save_obj_with_wrapper`` and project its camera-frame vertices with the intrinsics; and the
drawing half (``project_and_draw``, ``main``, :50-178), on the GPU through hm_mesh_overlay (hamer_yolo_amd/render.py): the
faces are filled by the rule of include/hamer_hip.h instead of cv2.fillConvexPoly, then blended as cv2.addWeighted does.

Formulated for whole meshes at once: the OBJ text is split into its record kinds in one pass and each kind is parsed
by one array conversion; the projection is one homogeneous product followed by one division."""
import argparse
import os
import re
import sys

import numpy as np

_FACE_CORNER = re.compile(rb"(-?\d+)(?:/\S*)?")


def load_intrinsics(txt_path):
    """reconstruct.py:14-25: the 3x3 matrix of a whitespace-separated text file, None (with a message) when it cannot
    be had."""
    try:
        return np.loadtxt(txt_path)
    except OSError:
        print(f"[Error] intrinsics file not found: {txt_path}")
    except ValueError as e:
        print(f"[Error] cannot read intrinsics: {e}")
    return None


def load_obj(obj_path):
    """reconstruct.py:27-47: ``(vertices (V,3) float64, faces (F,3) int, 0-based)``; ``(None, None)`` when the file is
    missing.  Only ``v`` and ``f`` records count; of a face corner ``i/t/n`` the vertex index ``i`` is taken, of a
    polygon its first three corners (what the reference keeps)."""
    try:
        with open(obj_path, "rb") as fh:
            records = fh.read().splitlines()
    except OSError:
        return None, None
    vert_text = [r[2:] for r in records if r[:2] == b"v "]
    face_text = [r[2:] for r in records if r[:2] == b"f "]
    verts = np.array([t.split()[:3] for t in vert_text], dtype=np.float64).reshape(len(vert_text), 3) if vert_text else np.array([])
    corners = [[int(m) for m in _FACE_CORNER.findall(t)[:3]] for t in face_text]
    faces = np.asarray(corners, dtype=np.int64) - 1 if corners else np.array([])
    return verts, faces


def project_vertices(vertices, faces, K):
    """reconstruct.py:55-66: integer pixel coordinates (V,2) int32 of the pinhole projection ``K @ v`` and the painter's
    order of the faces, farthest first (by mean corner depth).  A vertex at depth exactly 0 is moved to 1e-5, as the
    reference does before dividing."""
    pts = np.asarray(vertices, dtype=np.float64)
    depth = np.where(pts[:, 2] == 0.0, 1e-5, pts[:, 2])
    cam = np.column_stack([pts[:, :2], depth])
    homo = cam @ np.asarray(K, dtype=np.float64).T                      # rows [x', y', w']
    pixels = (homo[:, :2] / homo[:, 2:3]).astype(np.int32)
    face_depth = depth[np.asarray(faces, dtype=np.int64)].mean(axis=1)
    far_to_near = np.argsort(face_depth)[::-1]
    return pixels, far_to_near


def project_and_draw(image, vertices, faces, K, alpha=0.6, color=(0, 255, 0)):
    """reconstruct.py:50-86: ``image`` (H,W,3) uint8 BGR with the mesh filled in ``color`` (BGR) and blended ``alpha`` :
    ``1 - alpha``; a new array (the inputs are left unchanged; the reference moves z == 0 vertices in place)."""
    import torch
    from hamer_yolo_amd.render import overlay_frames
    img = np.ascontiguousarray(image, dtype=np.uint8)
    dev = torch.device("cuda", torch.cuda.current_device())
    mesh = {"frame": 0, "vertices": np.asarray(vertices, np.float64), "faces": np.asarray(faces, np.int64).astype(np.int32),
            "color": color}
    out = overlay_frames(torch.from_numpy(img[None]).to(dev), K, [mesh], alpha=alpha)
    return out[0].cpu().numpy()


def main(argv=None, frames_per_pass=None):
    """reconstruct.py:88-178: every image of ``--img_dir`` with an OBJ of the same name in ``--obj_dir`` -> ``--out_dir``
    ``<name>.jpg``; images without an OBJ are skipped.  Images are grouped by the size their headers give and drawn
    ``frames_per_pass`` at a time (default render.FRAMES_PER_PASS), one overlay call each; a pass's images and OBJs are read
    only when it is drawn and at most a few passes of encodes are pending, so memory does not grow with the folder.
    ``--ext`` (not in the reference) picks another PIL format."""
    from concurrent.futures import ThreadPoolExecutor

    import torch
    from hamer_yolo_amd.infer import _list_images
    from hamer_yolo_amd.render import (FRAMES_PER_PASS, PassWriter, _encode_threads, decode_pass, frame_size, overlay_frames,
                                       release_workspaces, size_passes)
    ap = argparse.ArgumentParser(description="project the OBJ meshes of a folder onto their images")
    ap.add_argument('--img_dir', type=str, required=True, help="folder of the original images")
    ap.add_argument('--obj_dir', type=str, required=True, help="folder of the OBJ files")
    ap.add_argument('--intrinsics', type=str, required=True, help="3x3 camera matrix txt (shared by every image)")
    ap.add_argument('--out_dir', type=str, required=True, help="output folder")
    ap.add_argument('--ext', type=str, default=".jpg", help="output extension (the reference writes .jpg)")
    args = ap.parse_args(argv)
    os.makedirs(args.out_dir, exist_ok=True)
    K = load_intrinsics(args.intrinsics)
    if K is None:
        sys.exit(1)
    img_paths = _list_images(args.img_dir)
    if not img_paths:
        print(f"[Error] no images in {args.img_dir}")
        sys.exit(1)
    dev = torch.device("cuda", torch.cuda.current_device())
    items = []                                         # (name, image path, OBJ path): paths only, nothing decoded yet
    for p in img_paths:
        name = os.path.splitext(os.path.basename(p))[0]
        obj_path = os.path.join(args.obj_dir, f"{name}.obj")
        if os.path.exists(obj_path):                   # a frame without hands has no OBJ
            items.append((name, p, obj_path))
    try:
        with ThreadPoolExecutor(_encode_threads()) as pool:
            writer = PassWriter(pool)
            sizes = list(pool.map(frame_size, [it[1] for it in items]))
            for i in (i for i, hw in enumerate(sizes) if hw is None):
                print(f"Skipping {items[i][0]}: Image load failed")
            for hw, part in size_passes(sizes, frames_per_pass or FRAMES_PER_PASS):
                meshes, keep = [], []
                for i in part:
                    vertices, faces = load_obj(items[i][2])
                    if vertices is None or len(vertices) == 0:
                        print(f"Skipping {items[i][0]}: OBJ empty or invalid")
                        continue
                    meshes.append({"vertices": vertices, "faces": np.asarray(faces, np.int64).astype(np.int32), "color": (0, 255, 0)})
                    keep.append(i)
                batch, ok = decode_pass(pool, [items[i][1] for i in keep], hw)
                if batch is None:
                    continue
                meshes = [dict(meshes[k], frame=n) for n, k in enumerate(ok)]
                out = overlay_frames(torch.from_numpy(batch).to(dev), K, meshes, alpha=0.6).cpu().numpy()
                writer.submit([(os.path.join(args.out_dir, items[keep[k]][0] + args.ext), out[n]) for n, k in enumerate(ok)])
            done = writer.close()
    finally:
        release_workspaces()
    print(f"{done}/{len(img_paths)} images drawn")
    return done


if __name__ == '__main__':
    main()
