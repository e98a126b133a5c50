"""Report what the camera sees of every predicted hand, and write it into the records.

    python -m hamer_yolo_amd.evaluate_visibility --pred <records dir> --intrinsics <K.txt or dir>
                                                 [--depth-maps DIR --unit U] [--masks DIR --label L] [--images DIR]
                                                 [--write-to DIR] [--json out.json]

``--pred`` holds the ``<stem>.npy`` hand records the folder job writes.  Per frame its hands are rendered together (the
z-buffer and label map of ``render.render_views``), and every hand gets a code per joint and per vertex -- VISIBLE, BEHIND the
near plane, OUTSIDE the frame, hidden by the hand itSELF, by the OTHER hand, by the SCENE (with ``--depth-maps``: something
the sensor saw in front of it) or OFF_MASK (with ``--masks``: its pixel does not carry ``--label``) -- and pixel counts: how
much of its silhouette is in the frame, in front, and clear.  The rules are in include/hamer_hip.h ("Visibility") and
DESIGN.md section 10.6, with what the flags cannot say.

The frame size comes from ``--images`` (headers only), else from the depth maps, else from the masks; one of the three is
needed.  A frame whose size, camera, depth map or mask is missing or of another size is skipped and named.

``--write-to DIR`` (which may be ``--pred``) writes every record again with, on every hand, ``joints_visible`` (21 uint8
codes), ``vertices_visible`` (778 uint8 codes), ``visible_share``, ``in_frame``, ``amodal_box``, ``modal_box`` and
``visibility_counts``; records of frames that cannot be scored are copied unchanged.
"""
from __future__ import annotations

import argparse
import glob
import json
import os
from concurrent.futures import ThreadPoolExecutor
from typing import Dict, List

import numpy as np

from .evaluate_depth import FRAMES_PER_PASS, _camera, depth_size, find_depth, load_cameras, load_depth

NEW_KEYS = ("joints_visible", "vertices_visible", "visible_share", "in_frame", "amodal_box", "modal_box", "visibility_counts")
SHARES = ("visible_share", "occluded_by_hand", "occluded_by_scene", "in_frame")


def _jobs(npy_folder, depth_folder, mask_folder, image_folder, rank: int, world: int) -> List[tuple]:
    """(stem, record path, record, hand sides in right, left order, depth path or None, frame path or None, mask path or None)
    of this rank's share of the records: ``evaluate_depth._jobs`` with every side input optional."""
    from .infer import _list_images, shard_paths
    frames = None
    if image_folder is not None:
        frames = {os.path.splitext(os.path.basename(p))[0]: p for p in _list_images(image_folder)}
    jobs = []
    for npy in shard_paths(sorted(glob.glob(os.path.join(npy_folder, "*.npy"))), rank, world):
        stem = os.path.splitext(os.path.basename(npy))[0]
        data = np.load(npy, allow_pickle=True).item()
        sides = [t for t in ("right", "left") if data.get(t) is not None]
        mask = None if mask_folder is None else os.path.join(mask_folder, stem + ".npy")
        jobs.append((stem, npy, data, sides, None if depth_folder is None else find_depth(depth_folder, stem),
                     None if frames is None else frames.get(stem), mask if mask is not None and os.path.exists(mask) else None))
    return jobs


def _passes(jobs, k_real, hamer, depth_folder, mask_folder, image_folder, unit, frames_per_pass, pool, skipped):
    """Yield per pass of equally sized frames ((H, W), job indices, sensor (n, H, W) uint16 or None, masks (n, H, W) uint8 or
    None, K (n, 3, 3)): ``evaluate_depth._passes`` with the depth maps and the masks optional and, without ``k_real``, the
    camera the records were made with (``render.default_camera``).  Frames that cannot be scored are named in one printed line
    each and appended to ``skipped``."""
    from . import render
    from .evaluate_masks import _load_mask

    def skip(i, why):
        print(f"Skipping {jobs[i][0]}: {why}")
        skipped.append(jobs[i][0])

    def size_of(i):
        j = jobs[i]
        return render.frame_size(j[5]) if image_folder is not None else depth_size(j[4] if depth_folder is not None else j[6])

    usable = []
    for i, j in enumerate(jobs):
        if not j[3]:
            continue                                                  # a record without hands has nothing to report
        if depth_folder is not None and j[4] is None:
            skip(i, f"no depth map in {depth_folder}")
        elif mask_folder is not None and j[6] is None:
            skip(i, f"no mask in {mask_folder}")
        elif image_folder is not None and j[5] is None:
            skip(i, f"no frame in {image_folder}")
        elif k_real is not None and _camera(k_real, j[0]) is None:
            skip(i, "no camera matrix")
        else:
            usable.append(i)
    sizes = list(pool.map(size_of, usable))
    for i, hw in zip(usable, sizes):
        if hw is None:
            skip(i, "unreadable size")
    for (H, W), idx in render.size_passes(sizes, frames_per_pass):
        part = [usable[k] for k in idx]
        depths = [None] * len(part) if depth_folder is None else list(pool.map(lambda i: load_depth(jobs[i][4], (H, W), unit), part))
        masks = [None] * len(part) if mask_folder is None else list(pool.map(lambda i: _load_mask(jobs[i][6], (H, W)), part))
        keep = []
        for n, i in enumerate(part):
            if depth_folder is not None and depths[n] is None:
                skip(i, f"no {H} x {W} 16-bit depth map {jobs[i][4]}")
            elif mask_folder is not None and masks[n] is None:
                skip(i, f"no {H} x {W} mask {jobs[i][6]}")
            else:
                keep.append(n)
        if not keep:
            continue
        cams = [_camera(k_real, jobs[part[n]][0]) if k_real is not None else render.default_camera(H, W, hamer.cfg) for n in keep]
        yield ((H, W), [part[n] for n in keep], np.stack([depths[n] for n in keep]) if depth_folder is not None else None,
               np.stack([masks[n] for n in keep]) if mask_folder is not None else None, np.stack(cams))


def _check(depth_folder, mask_folder, image_folder, label, unit):
    if depth_folder is None and mask_folder is None and image_folder is None:
        raise ValueError("visibility needs the frame size: give the frames (image_folder), depth maps or masks")
    if not 1 <= int(label) <= 255:
        raise ValueError(f"label must be in 1..255, got {label}")
    if not (np.isfinite(unit) and unit > 0):
        raise ValueError(f"unit must be finite and > 0, got {unit}")


def _scan(npy_folder, hamer, k_real, depth_folder, mask_folder, image_folder, unit, label, left_label, rank, world, frames_per_pass, options):
    """The common loop of ``score_folder`` and ``annotate_folder``: (jobs, {job index: {side: per-hand results}}, skipped).  Per
    pass of equally sized frames one MANO forward (joints and vertices) and one ``hand_visibility`` call, then one copy of each
    result to the host."""
    import torch
    from . import render
    from .hamer.utils import visibility as V
    _check(depth_folder, mask_folder, image_folder, label, unit)
    if left_label is not None and not 1 <= int(left_label) <= 255:
        raise ValueError(f"left_label must be in 1..255, got {left_label}")
    jobs = _jobs(npy_folder, depth_folder, mask_folder, image_folder, rank, world)
    dev = hamer.device
    faces = torch.as_tensor(np.asarray(hamer.mano.faces, np.int32), device=dev)
    found: Dict[int, Dict] = {}
    skipped: List[str] = []
    try:
        with ThreadPoolExecutor(render._encode_threads()) as pool:
            for (H, W), part, sensor, masks, K in _passes(jobs, k_real, hamer, depth_folder, mask_folder, image_folder, unit,
                                                          frames_per_pass, pool, skipped):
                hands = [(n, i, t) for n, i in enumerate(part) for t in jobs[i][3]]
                joints, verts = render.camera_joints_vertices(hamer, [jobs[i][2][t] for _, i, t in hands])
                meshes = [{"frame": n, "vertices": verts[j], "faces": faces, "faces_checked": True} for j, (n, _, _) in enumerate(hands)]
                r = V.hand_visibility(H, W, K, meshes, joints, views=len(part), unit=unit,
                                      sensor=None if sensor is None else torch.from_numpy(sensor).to(dev),
                                      mask=None if masks is None else torch.from_numpy(masks).to(dev),
                                      labels=None if masks is None else [int(label if t == "right" or left_label is None else left_label)
                                                                         for _, _, t in hands], **options)
                start = r["vertex_start"]
                vc, jc, cp, cx, bx = (r[k].cpu().numpy() for k in ("vertex_codes", "joint_codes", "counts_points", "counts_pixels", "boxes"))
                s = V.summary(cp, cx)
                for j, (_, i, t) in enumerate(hands):
                    found.setdefault(i, {})[t] = {"joints": jc[j].copy(), "vertices": vc[start[j]:start[j + 1]].copy(), "points": cp[j, 0].copy(),
                                                  "joint_points": cp[j, 1].copy(), "pixels": cx[j].copy(), "boxes": bx[j].copy(),
                                                  **{k: float(s[k][j]) for k in SHARES}}
    finally:
        render.release_workspaces()
        V.release_workspaces()
    return jobs, found, skipped


def score_folder(npy_folder, hamer, k_real, depth_folder=None, unit: float = 0.001, mask_folder=None, label: int = 3,
                 image_folder=None, rank: int = 0, world: int = 1, frames_per_pass: int = FRAMES_PER_PASS, left_label=None,
                 **options) -> Dict:
    """Visibility of every hand of every record of ``npy_folder``.  Streams as ``evaluate_depth.score_folder`` does: per pass
    of equally sized frames one MANO forward and one ``hamer.utils.visibility.hand_visibility`` call (render, point codes,
    coverage).  ``k_real``: (3, 3), {stem: (3, 3)}, or None for the camera the records were made with without intrinsics.
    ``depth_folder`` / ``unit``: sensor depth maps as ``evaluate_depth`` reads them; ``mask_folder`` / ``label``: label images
    (``left_label``: the label of left hands' pixels where the masks tell the hands apart; default: ``label`` for both).
    ``image_folder``: the frames, for their size (else the depth maps', else the masks').  ``options`` go to ``hand_visibility``
    (``vertex_tol_m``, ``joint_tol_m``, ``scene_tol_m``, ``window``, ``raw_range``).  Returns ``{'rows': [{stem, hand,
    visible_share, occluded_by_hand, occluded_by_scene, in_frame, joints_visible (count), vertex_counts [8], joint_counts [8],
    pixel_counts [8], amodal_box, modal_box}], 'hands', 'means': the folder means of the four shares over the hands where they
    are defined, 'skipped': [stems], 'n_skipped'}``.  The workspaces are released at the end."""
    jobs, found, skipped = _scan(npy_folder, hamer, k_real, depth_folder, mask_folder, image_folder, unit, label, left_label, rank, world,
                                 frames_per_pass, options)
    rows = []
    for i, job in enumerate(jobs):
        for t in job[3]:
            f = found.get(i, {}).get(t)
            if f is None:
                continue
            rows.append({"stem": job[0], "hand": t, **{k: f[k] for k in SHARES}, "joints_visible": int((f["joints"] == 0).sum()),
                         "vertex_counts": [int(v) for v in f["points"]], "joint_counts": [int(v) for v in f["joint_points"]],
                         "pixel_counts": [int(v) for v in f["pixels"]], "amodal_box": [int(v) for v in f["boxes"][:4]],
                         "modal_box": [int(v) for v in f["boxes"][4:]]})
    means = {}
    for k in SHARES:
        v = np.array([r[k] for r in rows], np.float64)
        means[k] = float(v[np.isfinite(v)].mean()) if np.isfinite(v).any() else float("nan")
    return {"rows": rows, "hands": len(rows), "means": means, "skipped": skipped, "n_skipped": len(skipped)}


def annotated_record(data: Dict, found: Dict) -> Dict:
    """The record with NEW_KEYS on every hand named in ``found`` (side -> the hand's results); every other key, and every
    other hand, keeps its object."""
    out = dict(data)
    for t in ("right", "left"):
        if data.get(t) is None or t not in found:
            continue
        f, h = found[t], dict(data[t])
        h["joints_visible"] = np.asarray(f["joints"], np.uint8)
        h["vertices_visible"] = np.asarray(f["vertices"], np.uint8)
        h["visible_share"], h["in_frame"] = float(f["visible_share"]), float(f["in_frame"])
        h["amodal_box"] = np.asarray(f["boxes"][:4], np.int32)
        h["modal_box"] = np.asarray(f["boxes"][4:], np.int32)
        h["visibility_counts"] = np.asarray(f["pixels"], np.int64)
        out[t] = h
    return out


def annotate_folder(npy_folder, out_folder, hamer, k_real, depth_folder=None, unit: float = 0.001, mask_folder=None,
                    label: int = 3, image_folder=None, rank: int = 0, world: int = 1, frames_per_pass: int = FRAMES_PER_PASS,
                    left_label=None, **options) -> Dict:
    """Write every record of ``npy_folder`` to ``out_folder`` (which may be the same folder) with NEW_KEYS on every hand:
    ``joints_visible`` (21,) uint8 and ``vertices_visible`` (778,) uint8 codes (``hamer.utils.visibility.CODES``),
    ``visible_share`` and ``in_frame`` (floats, NaN where undefined), ``amodal_box`` and ``modal_box`` (4,) int32 x1, y1, x2, y2
    (-1 without pixels) and ``visibility_counts`` (8,) int64 (``PIXEL_COUNT_NAMES``).  Arguments as ``score_folder``.  The record
    of a frame that cannot be scored, and a record without hands, is copied unchanged.  Returns ``{'records', 'hands',
    'annotated', 'skipped', 'n_skipped'}``."""
    os.makedirs(out_folder, exist_ok=True)
    jobs, found, skipped = _scan(npy_folder, hamer, k_real, depth_folder, mask_folder, image_folder, unit, label, left_label, rank, world,
                                 frames_per_pass, options)
    n_hands = n_done = 0
    for i, job in enumerate(jobs):
        n_hands += len(job[3])
        n_done += len(found.get(i, {}))
        dst = os.path.join(out_folder, job[0] + ".npy")
        if i in found:
            np.save(dst, annotated_record(job[2], found[i]))
        elif os.path.abspath(dst) != os.path.abspath(job[1]):
            with open(job[1], "rb") as src, open(dst, "wb") as out:
                out.write(src.read())
    return {"records": len(jobs), "hands": n_hands, "annotated": n_done, "skipped": skipped, "n_skipped": len(skipped)}


def format_line(result: Dict) -> str:
    m = result["means"]
    return (f"{result['hands']} hands: visible {m['visible_share']:.4f}, behind another hand {m['occluded_by_hand']:.4f}, behind the "
            f"scene {m['occluded_by_scene']:.4f}, in frame {m['in_frame']:.4f}; skipped {result['n_skipped']}")


def _parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description="report which joints, vertices and pixels of every predicted hand the camera sees")
    ap.add_argument('--pred', type=str, required=True, help="folder of .npy hand records")
    ap.add_argument('--intrinsics', type=str, required=True, help="3x3 camera matrix txt the records were made with, or a folder of <stem>.txt")
    ap.add_argument('--depth-maps', type=str, default=None, metavar="DIR",
                    help="folder of <stem>.png (16-bit) or <stem>.npy sensor depth maps, registered to the frames: what the sensor saw in front of a hand hides it")
    ap.add_argument('--unit', type=float, default=0.001, metavar="U", help="with --depth-maps: metres per raw unit (default 0.001: millimetres)")
    ap.add_argument('--masks', type=str, default=None, metavar="DIR", help="folder of <stem>.npy label images: a hand pixel that does not carry --label is off the mask")
    ap.add_argument('--label', type=int, default=3, metavar="L", help="with --masks: the mask value of hand pixels (the reference's masks use 3)")
    ap.add_argument('--images', type=str, default=None, metavar="DIR", help="folder of the frames (headers only: the frame size)")
    ap.add_argument('--write-to', type=str, default=None, metavar="DIR", help="also write the records with the visibility keys into DIR")
    ap.add_argument('--json', type=str, default=None, help="also write the result, per-hand rows included, to this file")
    ap.add_argument('--ckpt', type=str, default=None, help="hamer.ckpt path or synthetic:<seed> (default: config/hamer_config.py); only its MANO model is used")
    return ap


def main(argv=None):
    ap = _parser()
    args = ap.parse_args(argv)
    if not (np.isfinite(args.unit) and args.unit > 0):
        ap.error("--unit must be > 0")
    if args.unit != 0.001 and not args.depth_maps:
        ap.error("--unit needs --depth-maps DIR")
    if args.label != 3 and not args.masks:
        ap.error("--label needs --masks DIR")
    if not (args.depth_maps or args.masks or args.images):
        ap.error("the frame size is needed: give --images, --depth-maps or --masks")
    from .config.hamer_config import hamer_opt
    from .infer import hamer_inference
    if args.ckpt:
        hamer_opt.ckpt_path = args.ckpt
    k_real = load_cameras(args.intrinsics)
    if k_real is None:
        ap.error(f"--intrinsics {args.intrinsics}: no 3x3 matrix")
    hamer = hamer_inference(hamer_opt)
    kw = dict(depth_folder=args.depth_maps, unit=args.unit, mask_folder=args.masks, label=args.label, image_folder=args.images)
    result = score_folder(args.pred, hamer, k_real, **kw)
    if args.write_to:
        result["annotate"] = annotate_folder(args.pred, args.write_to, hamer, k_real, **kw)
        print(f"{result['annotate']['annotated']} of {result['annotate']['hands']} hands annotated into {args.write_to}")
    if args.json:
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)
    print(format_line(result))
    for s in result["skipped"]:
        print(f"skipped: {s}")
    return result


if __name__ == '__main__':
    main()
