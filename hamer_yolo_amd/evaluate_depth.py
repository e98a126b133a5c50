"""Score predicted hand depth against per-frame sensor depth maps, and shift the hands onto them.

    python -m hamer_yolo_amd.evaluate_depth --pred <records dir> --depth-maps <depth dir> --intrinsics <K.txt or dir>
                                            [--depth-scale 0.001] [--masks DIR --label 3] [--images DIR] [--json out.json]
                                            [--refine-to DIR [--refine-mode ray|rigid]]

``--pred`` holds the ``<stem>.npy`` hand records the folder job writes and ``--depth-maps`` one depth map per frame, registered
to the colour frame: ``<stem>.png`` (16-bit, raw units of ``--depth-scale`` metres) or ``<stem>.npy`` (uint16: raw units;
float: metres).  0 means no measurement.  ``--intrinsics`` is required -- a residual under a made-up camera means nothing --
and is one 3x3 matrix or a folder of ``<stem>.txt``.  Per hand the z-buffered render of its mesh is compared with the sensor
over the pixels the hand covers (with ``--masks``: only where the frame's label image carries ``--label``): the residual
``sensor - predicted`` is positive when the hand was predicted too near.  The rule is in include/hamer_hip.h ("Depth
residuals") and DESIGN.md section 10.3.

``--refine-to DIR`` writes the records again with every hand moved along the ray of its origin by the median residual (two
rounds of render, score, shift: ``hamer.utils.depth_eval.refine_cam_t``); the records gain ``cam_t_unrefined``,
``depth_residual_m``, ``depth_pixels`` and ``depth_refined``.  ``--refine-mode rigid`` goes on from there with a rigid
point-to-plane fit of every hand to the sensor's surface about its wrist joint (six rounds of render, fit, move:
``hamer.utils.depth_eval.fit_rigid``): the rotation is folded into ``pose_global`` (and ``theta[:3]``),
the translation into ``cam_t``, and the records also gain ``pose_global_unrefined``, ``depth_fit_rms_m``, ``depth_fit_pixels``
and ``depth_fit``.

A depth map takes the size of its frame (``--images``: the frames' headers; without, the depth map's own size is the frame's).
A frame whose depth map, mask or camera is missing or of another size is skipped and named.
"""
from __future__ import annotations

import argparse
import glob
import json
import os
from concurrent.futures import ThreadPoolExecutor
from typing import Dict, List, Optional

import numpy as np

FRAMES_PER_PASS = 16
THRESHOLDS_M = (0.005, 0.010, 0.020)
NEW_KEYS = ("cam_t_unrefined", "depth_residual_m", "depth_pixels", "depth_refined")
FIT_KEYS = ("pose_global_unrefined", "depth_fit_rms_m", "depth_fit_pixels", "depth_fit")      # --refine-mode rigid adds these
REFINE_MODES = ("ray", "rigid")


def find_depth(depth_folder: str, stem: str) -> Optional[str]:
    for ext in (".png", ".npy"):
        p = os.path.join(depth_folder, stem + ext)
        if os.path.exists(p):
            return p
    return None


def depth_size(path: str) -> Optional[tuple]:
    """(H, W) of a depth map from its header; None when unreadable."""
    from . import render
    if path.endswith(".npy"):
        try:
            a = np.load(path, mmap_mode="r", allow_pickle=False)
            return (int(a.shape[0]), int(a.shape[1])) if a.ndim == 2 else None
        except Exception:
            return None
    return render.frame_size(path)


def load_depth(path: str, hw: tuple, unit: float) -> Optional[np.ndarray]:
    """The (H, W) uint16 raw depth at ``path``; None when it is unreadable or of another size.  A 16-bit PNG and a uint16
    ``.npy`` hold raw units; a float ``.npy`` holds metres: rint(m / unit), clipped to 0..65535 (NaN: 0)."""
    try:
        if path.endswith(".npy"):
            a = np.load(path, allow_pickle=False)
        else:
            from PIL import Image
            with Image.open(path) as im:
                if im.mode not in ("I;16", "I;16L", "I;16B", "I"):
                    return None
                a = np.asarray(im)
    except Exception:
        return None
    if a.ndim != 2 or tuple(a.shape) != tuple(hw):
        return None
    if a.dtype.kind == "f":
        a = np.clip(np.rint(np.nan_to_num(a.astype(np.float64), nan=0.0, posinf=0.0, neginf=0.0) / float(unit)), 0, 65535)
    elif a.dtype.kind in "iu":
        a = np.clip(a, 0, 65535)
    else:
        return None
    return np.ascontiguousarray(a.astype(np.uint16))


def load_cameras(path: str):
    """``--intrinsics``: a 3x3 matrix file, or a folder of ``<stem>.txt`` (-> {stem: K})."""
    from .infer import load_intrinsics
    if os.path.isdir(path):
        return {os.path.splitext(os.path.basename(p))[0]: load_intrinsics(p) for p in sorted(glob.glob(os.path.join(path, "*.txt")))}
    return load_intrinsics(path)


def _camera(k_real, stem: str) -> Optional[np.ndarray]:
    k = k_real.get(stem) if isinstance(k_real, dict) else k_real
    return None if k is None else np.asarray(k, np.float64)


def _jobs(npy_folder, depth_folder, image_folder, rank: int, world: int) -> List[tuple]:
    """(stem, record path, record, hand sides in right, left order, depth path, frame path or None) of this rank's share of the
    records.  ``render._record_jobs`` keys the records on their frames; here they are keyed on their depth maps, which may be
    ``.npy`` files, so the records are listed directly."""
    from .infer import _list_images, shard_paths
    frames = None
    if image_folder is not None:
        frames = {os.path.splitext(os.path.basename(p))[0]: p for p in _list_images(image_folder)}
    jobs = []
    for npy in shard_paths(sorted(glob.glob(os.path.join(npy_folder, "*.npy"))), rank, world):
        stem = os.path.splitext(os.path.basename(npy))[0]
        data = np.load(npy, allow_pickle=True).item()
        sides = [t for t in ("right", "left") if data.get(t) is not None]
        jobs.append((stem, npy, data, sides, find_depth(depth_folder, stem), None if frames is None else frames.get(stem)))
    return jobs


def _passes(jobs, k_real, depth_folder, mask_folder, image_folder, unit, frames_per_pass, pool, skipped):
    """Yield per pass of equally sized frames ((H, W), job indices, sensor (n, H, W) uint16, masks (n, H, W) uint8 or None,
    K (n, 3, 3)); frames that cannot be scored are named in one printed line each and appended to ``skipped``."""
    from . import render
    from .evaluate_masks import _load_mask

    def skip(i, why):
        print(f"Skipping {jobs[i][0]}: {why}")
        skipped.append(jobs[i][0])

    usable = []
    for i, j in enumerate(jobs):
        if not j[3]:
            continue                                                  # a record without hands has nothing to score or move
        if j[4] is None:
            skip(i, f"no depth map in {depth_folder}")
        elif image_folder is not None and j[5] is None:
            skip(i, f"no frame in {image_folder}")
        elif _camera(k_real, j[0]) is None:
            skip(i, "no camera matrix")
        else:
            usable.append(i)
    sizes = list(pool.map(lambda i: render.frame_size(jobs[i][5]) if image_folder is not None else depth_size(jobs[i][4]), usable))
    for i, hw in zip(usable, sizes):
        if hw is None:
            skip(i, "unreadable size")
    for (H, W), idx in render.size_passes(sizes, frames_per_pass):
        part = [usable[k] for k in idx]
        depths = list(pool.map(lambda i: load_depth(jobs[i][4], (H, W), unit), part))
        masks = [None] * len(part)
        if mask_folder is not None:
            masks = list(pool.map(lambda i: _load_mask(os.path.join(mask_folder, jobs[i][0] + ".npy"), (H, W)), part))
        keep = []
        for n, i in enumerate(part):
            if depths[n] is None:
                skip(i, f"no {H} x {W} 16-bit depth map {jobs[i][4]}")
            elif mask_folder is not None and masks[n] is None:
                skip(i, f"no {H} x {W} mask {os.path.join(mask_folder, jobs[i][0] + '.npy')}")
            else:
                keep.append(n)
        if not keep:
            continue
        yield ((H, W), [part[n] for n in keep], np.stack([depths[n] for n in keep]),
               np.stack([masks[n] for n in keep]) if mask_folder is not None else None,
               np.stack([_camera(k_real, jobs[part[n]][0]) for n in keep]))


def _check(k_real, label, unit):
    if k_real is None:
        raise ValueError("depth scoring needs the camera intrinsics the records were made with (k_real)")
    if not 1 <= int(label) <= 255:
        raise ValueError(f"label must be in 1..255, got {label}")
    if not (np.isfinite(unit) and unit > 0):
        raise ValueError(f"unit must be finite and > 0, got {unit}")


def score_folder(npy_folder, depth_folder, hamer, k_real, unit: float = 0.001, mask_folder=None, label: int = 3,
                 image_folder=None, rank: int = 0, world: int = 1, frames_per_pass: int = FRAMES_PER_PASS) -> Dict:
    """Score every hand of every record of ``npy_folder`` against its frame's depth map in ``depth_folder``.  Streams as
    ``evaluate_masks.score_folder`` does: per pass of equally sized frames one MANO forward, one ``render_views`` call (depth
    and mesh_id), one upload of the pass's depth maps (and masks) and ONE hm_depth_residuals call with one query per hand.
    ``k_real``: (3, 3), or {stem: (3, 3)}.  ``mask_folder``: only pixels whose ``<stem>.npy`` label equals ``label`` count.
    ``image_folder``: take the frame sizes from the frames' headers (default: from the depth maps).  ``rank`` / ``world``: this
    process scores ``shard_paths(records, rank, world)``.  Returns ``{'rows': [{stem, hand, median_m, mean_abs_m, inliers,
    measured, occluded, counts}], 'hands', 'scored', 'median_abs_mm', 'mean_abs_mm', 'inliers', 'measured', 'occluded',
    'skipped': [stems], 'n_skipped', 'unit', 'label'}`` (``DepthEvaluator.result``; NaN when nothing could be scored).  The
    workspaces are released at the end."""
    import torch
    from . import render
    from .hamer.utils import depth_eval as DE
    _check(k_real, label, unit)
    jobs = _jobs(npy_folder, depth_folder, image_folder, rank, world)
    dev = hamer.device
    faces = torch.as_tensor(np.asarray(hamer.mano.faces, np.int32), device=dev)
    ev = DE.DepthEvaluator(unit=unit, thresholds_m=THRESHOLDS_M)
    names, skipped = [], []
    try:
        with ThreadPoolExecutor(render._encode_threads()) as pool:
            for (H, W), part, sensor, masks, K in _passes(jobs, k_real, depth_folder, mask_folder, image_folder, unit,
                                                          frames_per_pass, pool, skipped):
                hands = [(n, jobs[i][2][t]) for n, i in enumerate(part) for t in jobs[i][3]]
                verts = render.camera_vertices(hamer, [h for _, h in hands])
                meshes = [{"frame": n, "vertices": verts[j], "faces": faces} for j, (n, _) in enumerate(hands)]
                r = render.render_views(H, W, K, meshes, outputs=("depth", "mesh_id"), views=len(part), device=dev)
                ev(r["depth"], r["mesh_id"], torch.from_numpy(sensor).to(dev), np.arange(len(hands)), len(hands),
                   mask=None if masks is None else torch.from_numpy(masks).to(dev),
                   labels=None if masks is None else [int(label)] * len(hands))
                names += [(jobs[i][0], t) for i in part for t in jobs[i][3]]
        per = ev.per_query()
        counts = ev.counts()
        summary = ev.result() if ev.n else DE.dataset_summary(np.zeros((0, ev.bins), np.int64), np.zeros((0, 8), np.int64), ev.bin_m,
                                                              THRESHOLDS_M)
    finally:
        render.release_workspaces()
        DE.release_workspaces()
    rows = [{"stem": s, "hand": t, "median_m": float(per["median"][n]), "mean_abs_m": float(per["mean_abs"][n]),
             "inliers": [float(v) for v in per["inliers"][n]], "measured": float(per["measured"][n]),
             "occluded": float(per["occluded"][n]), "counts": [int(v) for v in counts[n, :6]]} for n, (s, t) in enumerate(names)]
    return {"rows": rows, **summary, "skipped": skipped, "n_skipped": len(skipped), "unit": float(unit), "label": int(label)}


def _refined_record(data: Dict, moved: Dict) -> Dict:
    """The record with the new keys on every hand; ``moved``: side -> (cam_t, median, pixels, updated) of the scored hands."""
    out = dict(data)
    for t in ("right", "left"):
        if data.get(t) is None:
            continue
        h = dict(data[t])
        old = h["cam_t"]
        h.setdefault("cam_t_unrefined", old)
        h["depth_residual_m"], h["depth_pixels"], h["depth_refined"] = float("nan"), 0, False
        if t in moved:
            cam_t, median, pixels, updated = moved[t]
            if updated:
                h["cam_t"] = np.asarray(cam_t, np.asarray(old).dtype).reshape(np.asarray(old).shape)
            h["depth_residual_m"], h["depth_pixels"], h["depth_refined"] = float(median), int(pixels), bool(updated)
        out[t] = h
    return out


def _exp_so3(w) -> np.ndarray:
    """Rodrigues' formula, fp64: a rotation vector (3,) -> (3, 3)."""
    w = np.asarray(w, np.float64).reshape(3)
    th = float(np.sqrt((w * w).sum()))
    Kx = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    a, b = (1.0 - th * th / 6.0, 0.5 - th * th / 24.0) if th < 1e-8 else (np.sin(th) / th, (1.0 - np.cos(th)) / (th * th))
    return np.eye(3) + a * Kx + b * (Kx @ Kx)


def _log_so3(R) -> np.ndarray:
    """The rotation vector (3,) of a rotation matrix, fp64; angles up to pi (at pi the axis comes from R + I)."""
    R = np.asarray(R, np.float64)
    w = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s, c = 0.5 * float(np.sqrt((w * w).sum())), 0.5 * (float(np.trace(R)) - 1.0)
    th = float(np.arctan2(s, c))
    if s >= 1e-6:
        return w * (th / (2.0 * s))
    if c > 0:
        return 0.5 * w
    col = (R + np.eye(3))[:, int(np.argmax(np.diag(R)))]
    return col / np.linalg.norm(col) * th


def fold_rotation(pose_global, rotation, is_right: bool) -> np.ndarray:
    """The global orientation (3,) fp64 of a record whose placed mesh was turned by ``rotation`` (3, 3) about its placed wrist
    joint.  MANO turns the hand about that joint, so for a right hand the new orientation is log(R exp(pose_global)); a left
    hand's mesh is mirrored by M = diag(-1, 1, 1) after MANO, so R acts on MANO's output as M R M."""
    M = np.diag([1.0 if is_right else -1.0, 1.0, 1.0])
    return _log_so3(M @ np.asarray(rotation, np.float64) @ M @ _exp_so3(pose_global))


def _fitted_record(data: Dict, moved: Dict, fitted: Dict) -> Dict:
    """``_refined_record`` plus FIT_KEYS on every hand; ``fitted``: side -> (rotation (3, 3), rms, pixels, applied) of the
    fitted hands.  An applied rotation goes into ``pose_global`` and, where the record has one, ``theta[:3]``."""
    out = _refined_record(data, moved)
    for t in ("right", "left"):
        if out.get(t) is None:
            continue
        h = out[t]
        old = h["pose_global"]
        h.setdefault("pose_global_unrefined", old)
        h["depth_fit_rms_m"], h["depth_fit_pixels"], h["depth_fit"] = float("nan"), 0, False
        if t in fitted:
            R, rms, pixels, applied = fitted[t]
            if applied:
                new = fold_rotation(old, R, bool(h["is_right"]))
                h["pose_global"] = new.astype(np.asarray(old).dtype).reshape(np.asarray(old).shape)
                if h.get("theta") is not None:
                    theta = np.array(h["theta"])
                    theta.reshape(-1)[:3] = h["pose_global"].reshape(-1)
                    h["theta"] = theta
            h["depth_fit_rms_m"], h["depth_fit_pixels"], h["depth_fit"] = float(rms), int(pixels), bool(applied)
    return out


def refine_folder(npy_folder, depth_folder, out_folder, hamer, k_real, unit: float = 0.001, mask_folder=None, label: int = 3,
                  iterations: int = 2, min_pixels: int = 200, min_fraction: float = 0.25, image_folder=None, rank: int = 0,
                  world: int = 1, frames_per_pass: int = FRAMES_PER_PASS, mode: str = "ray", fit_iterations: int = 6) -> Dict:
    """Write every record of ``npy_folder`` to ``out_folder`` (which may be the same folder) with its hands moved along the
    rays of their origins onto the depth maps: ``refine_cam_t`` per pass, with the pass structure and arguments of
    ``score_folder``.  Every hand gains ``cam_t_unrefined`` (its cam_t before), ``depth_residual_m`` (the last median; NaN
    when it was not scored), ``depth_pixels`` (the valid pixels behind it) and ``depth_refined``; every other key keeps its
    type and, for a hand that was not moved, its bytes.  A record whose frame is skipped is written with those defaults.
    ``mode='rigid'`` goes on from the ray rounds with ``fit_iterations`` rounds of ``fit_rigid`` about every hand's wrist
    joint (joint 0 of MANO, mirrored for a left hand, plus cam_t) and folds the fit into the record: ``pose_global`` (and
    ``theta[:3]``) takes the rotation (``fold_rotation``), ``cam_t`` the translation, and every hand also gains FIT_KEYS:
    ``pose_global_unrefined``, ``depth_fit_rms_m`` (the last point-to-plane rms; NaN when no pixel was used),
    ``depth_fit_pixels`` and ``depth_fit`` (a rigid step was applied).  ``mode='ray'`` writes what it always wrote.
    Returns ``{'records', 'hands', 'refined', 'skipped', 'n_skipped'}``, in rigid mode also ``'fitted'``."""
    import torch
    from . import render
    from .hamer.utils import depth_eval as DE
    from .infer import mano_hand_joints_vertices, mano_hand_vertices
    _check(k_real, label, unit)
    if mode not in REFINE_MODES:
        raise ValueError(f"mode must be one of {REFINE_MODES}, got {mode!r}")
    os.makedirs(out_folder, exist_ok=True)
    jobs = _jobs(npy_folder, depth_folder, image_folder, rank, world)
    dev = hamer.device
    faces = torch.as_tensor(np.asarray(hamer.mano.faces, np.int32), device=dev)
    moved: Dict[int, Dict] = {}
    fitted: Dict[int, Dict] = {}
    skipped: List[str] = []
    n_hands = n_refined = n_fitted = 0
    try:
        with ThreadPoolExecutor(render._encode_threads()) as pool:
            for (H, W), part, sensor, masks, K in _passes(jobs, k_real, depth_folder, mask_folder, image_folder, unit,
                                                          frames_per_pass, pool, skipped):
                hands = [(n, i, t) for n, i in enumerate(part) for t in jobs[i][3]]
                recs = [jobs[i][2][t] for _, i, t in hands]
                sign = torch.tensor([[1.0, 1.0, 1.0] if h["is_right"] else [-1.0, 1.0, 1.0] for h in recs], device=dev)
                cam_t = torch.tensor(np.stack([np.asarray(h["cam_t"], np.float32).reshape(3) for h in recs]), device=dev)
                if mode == "rigid":
                    joints, verts = mano_hand_joints_vertices(hamer, recs)
                    pivot = (joints[:, 0, :] * sign).to(torch.float64) + cam_t.to(torch.float64)
                    r = DE.fit_rigid(H, W, K, verts * sign[:, None, :], faces, cam_t, pivot, [n for n, _, _ in hands],
                                     torch.from_numpy(sensor).to(dev), unit=unit, ray_iterations=iterations,
                                     iterations=fit_iterations, min_pixels=min_pixels, min_fraction=min_fraction,
                                     mask=None if masks is None else torch.from_numpy(masks).to(dev),
                                     labels=None if masks is None else [int(label)] * len(hands))
                    new, med, pix, upd, rot, rms, used, fit = (r[k].cpu().numpy() for k in ("cam_t", "median", "valid", "updated",
                                                                                            "rotation", "rms", "used", "fitted"))
                    for j, (_, i, t) in enumerate(hands):
                        moved.setdefault(i, {})[t] = (new[j], med[j], pix[j], upd[j])
                        fitted.setdefault(i, {})[t] = (rot[j], rms[j], used[j], fit[j])
                    n_refined += int(upd.sum())
                    n_fitted += int(fit.sum())
                    continue
                verts = mano_hand_vertices(hamer, recs) * sign[:, None, :]
                r = DE.refine_cam_t(H, W, K, verts, faces, cam_t, [n for n, _, _ in hands], torch.from_numpy(sensor).to(dev),
                                    unit=unit, iterations=iterations, min_pixels=min_pixels, min_fraction=min_fraction,
                                    mask=None if masks is None else torch.from_numpy(masks).to(dev),
                                    labels=None if masks is None else [int(label)] * len(hands))
                new, med, pix, upd = (r[k].cpu().numpy() for k in ("cam_t", "median", "valid", "updated"))
                for j, (_, i, t) in enumerate(hands):
                    moved.setdefault(i, {})[t] = (new[j], med[j], pix[j], upd[j])
                n_refined += int(upd.sum())
        for i, job in enumerate(jobs):
            n_hands += len(job[3])
            rec = _refined_record(job[2], moved.get(i, {})) if mode == "ray" else _fitted_record(job[2], moved.get(i, {}), fitted.get(i, {}))
            np.save(os.path.join(out_folder, job[0] + ".npy"), rec)
    finally:
        render.release_workspaces()
        DE.release_workspaces()
        DE.release_fit_workspaces()
    out = {"records": len(jobs), "hands": n_hands, "refined": n_refined, "skipped": skipped, "n_skipped": len(skipped)}
    if mode == "rigid":
        out["fitted"] = n_fitted
    return out


def format_line(result: Dict) -> str:
    inl = ", ".join(f"{k} {v:.4f}" for k, v in result["inliers"].items())
    return (f"{result['hands']} hands, {result['scored']} scored: median |residual| {result['median_abs_mm']:.2f} mm, mean |residual| "
            f"{result['mean_abs_mm']:.2f} mm; inliers {inl}; measured {result['measured']:.4f}, occluded {result['occluded']:.4f}; "
            f"skipped {result['n_skipped']}")


def _parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description="score predicted hand depth against sensor depth maps, and shift the hands onto them")
    ap.add_argument('--pred', type=str, required=True, help="folder of .npy hand records to score")
    ap.add_argument('--depth-maps', type=str, required=True, help="folder of <stem>.png (16-bit) or <stem>.npy depth maps, registered to the frames")
    ap.add_argument('--intrinsics', type=str, required=True,
                    help="3x3 camera matrix txt the records were made with, or a folder of <stem>.txt (required: a residual under a made-up camera means nothing)")
    ap.add_argument('--depth-scale', type=float, default=0.001, help="metres per raw unit of the 16-bit depth maps (default 0.001: millimetres)")
    ap.add_argument('--masks', type=str, default=None, help="folder of <stem>.npy label images: only pixels that carry --label count")
    ap.add_argument('--label', type=int, default=3, help="with --masks: the mask value of hand pixels (the reference's masks use 3)")
    ap.add_argument('--images', type=str, default=None, help="folder of the frames (headers only: the size a depth map must have)")
    ap.add_argument('--refine-to', type=str, default=None, metavar="DIR", help="also write the records with depth-refined cam_t into DIR")
    ap.add_argument('--refine-mode', type=str, default="ray", choices=REFINE_MODES,
                    help="with --refine-to: ray (default) moves every hand along the ray of its origin; rigid goes on with a "
                         "point-to-plane fit of all six degrees of freedom about the wrist and folds it into pose_global and cam_t")
    ap.add_argument('--json', type=str, default=None, help="also write the result, per-hand rows included, to this file")
    ap.add_argument('--ckpt', type=str, default=None, help="hamer.ckpt path or synthetic:<seed> (default: config/hamer_config.py); only its MANO model is used")
    return ap


def main(argv=None):
    ap = _parser()
    args = ap.parse_args(argv)
    if not (np.isfinite(args.depth_scale) and args.depth_scale > 0):
        ap.error("--depth-scale must be > 0")
    from .config.hamer_config import hamer_opt
    from .infer import hamer_inference
    if args.ckpt:
        hamer_opt.ckpt_path = args.ckpt
    k_real = load_cameras(args.intrinsics)
    if k_real is None:
        ap.error(f"--intrinsics {args.intrinsics}: no 3x3 matrix")
    hamer = hamer_inference(hamer_opt)
    kw = dict(unit=args.depth_scale, mask_folder=args.masks, label=args.label, image_folder=args.images)
    result = score_folder(args.pred, args.depth_maps, hamer, k_real, **kw)
    if args.refine_to:
        result["refine"] = refine_folder(args.pred, args.depth_maps, args.refine_to, hamer, k_real, mode=args.refine_mode, **kw)
        print(f"{result['refine']['refined']} of {result['refine']['hands']} hands refined into {args.refine_to}")
    if args.json:
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)
    print(format_line(result))
    for s in result["skipped"]:
        print(f"skipped: {s}")
    return result


if __name__ == '__main__':
    main()
