"""Score predicted hand meshes against per-frame label masks: region similarity J and contour accuracy F.

    python -m hamer_yolo_amd.evaluate_masks --pred <records dir> --images <frames dir> --masks <mask dir>
                                            [--label 3] [--bound-th 0.008] [--intrinsics K.txt] [--json out.json]
                                            [--refine-to DIR [--fit-rounds 6] [--fit-radius R]]

``--pred`` holds the ``<stem>.npy`` hand records the folder job writes, ``--images`` the frames they were made from (only
their headers are read, for the size) and ``--masks`` one ``<stem>.npy`` label image per frame, ``--label`` on hand pixels:
the masks ``process_batch_manopara_with_mask`` / ``get_bbox_from_npy`` read and ``--hand-maps`` writes.  Per frame the
silhouette of ALL its predicted hands (the z-buffered renderer's coverage) is scored against the pixels that carry the label,
because such masks carry one hand label and do not tell the hands apart.  Masks with a label per hand can be scored per hand
through ``hamer.utils.mask_eval.mask_counts`` with one query per hand.

J is intersection over union; F is the harmonic mean of boundary precision and recall within ``bound_th`` of the image
diagonal (``bound_radius``: 18 pixels at 1080 x 1920).  The rule is the DAVIS benchmark's J and F written from their
definition (include/hamer_hip.h); it is unpinned against DAVIS's own script.

``--refine-to DIR`` writes the records again with every hand fitted to its frame's mask in four degrees of freedom -- shift
in the image plane, scale (depth) and rotation about the viewing axis -- by ``--fit-rounds`` rounds of render, contour
alignment and move about the wrist joint (``hamer.utils.mask_eval.fit_contour``; ``--fit-radius``: the
search radius in pixels, default ``fit_radius``: 36 at 1080 x 1920).  The rotation is folded into ``pose_global`` (and
``theta[:3]``), the motion of the wrist into ``cam_t``; the records gain ``cam_t_unrefined``, ``pose_global_unrefined``,
``mask_fit_rms_px``, ``mask_fit_pixels`` and ``mask_fit``.  J and F of the folder before and after are printed and written.

A record without hands but with a mask is scored with an empty prediction.  A frame without a mask file, or whose mask has
another size than the frame, is skipped and named.
"""
from __future__ import annotations

import argparse
import json
import os
from concurrent.futures import ThreadPoolExecutor
from typing import Dict, Optional

import numpy as np

FRAMES_PER_PASS = 16
FIT_KEYS = ("cam_t_unrefined", "pose_global_unrefined", "mask_fit_rms_px", "mask_fit_pixels", "mask_fit")     # --refine-to adds these
FIT_ROUNDS = 6


def _load_mask(path: str, hw: tuple) -> Optional[np.ndarray]:
    """The (H, W) uint8 label image at ``path``; None when it is missing, unreadable or of another size."""
    if not os.path.exists(path):
        return None
    try:
        m = np.load(path, allow_pickle=False)
    except Exception:
        return None
    if m.ndim != 2 or tuple(m.shape) != tuple(hw) or m.dtype.kind not in "uib":
        return None
    if m.dtype != np.uint8:                          # wider labels: what does not fit a byte is no hand label (1..255)
        m = np.where((m >= 0) & (m <= 255), m, 0).astype(np.uint8)
    return np.ascontiguousarray(m)


def score_folder(image_folder, npy_folder, mask_folder, hamer, k_real=None, label: int = 3, bound_th: float = 0.008,
                 rank: int = 0, world: int = 1, frames_per_pass: int = FRAMES_PER_PASS) -> Dict:
    """Score the records of ``npy_folder`` against ``mask_folder``'s ``<stem>.npy`` label images.  Streams as
    ``render.hand_maps_folder`` does: per pass of equally sized frames one MANO forward, one ``render_views`` call, one upload
    of the pass's masks and one hm_mask_score call with one query per frame -- the union of the frame's hands against
    ``label``.  ``k_real`` None: the camera the records were made with.  ``rank`` / ``world``: this process scores
    ``shard_paths(records, rank, world)``.  Returns ``{'frames': {stem: {J, F, precision, recall}}, 'j_mean', 'j_recall',
    'f_mean', 'f_recall', 'jf_mean', 'n', 'skipped': [stems], 'n_skipped', 'label', 'bound_th'}`` (the means are NaN when no
    frame could be scored).  The workspaces are released at the end."""
    import torch
    from . import render
    from .hamer.utils import mask_eval as ME
    if not 1 <= int(label) <= 255:
        raise ValueError(f"label must be in 1..255, got {label}")
    jobs = render._record_jobs(image_folder, npy_folder, rank, world, keep_empty=True)
    dev = hamer.device
    faces = torch.as_tensor(np.asarray(hamer.mano.faces, np.int32), device=dev)
    ev = ME.MaskEvaluator()
    stems, skipped = [], []
    try:
        with ThreadPoolExecutor(render._encode_threads()) as pool:
            sizes = list(pool.map(render.frame_size, [j[1] for j in jobs]))
            for i in (i for i, hw in enumerate(sizes) if hw is None):
                print(f"Skipping {jobs[i][0]}: image load failed")
                skipped.append(jobs[i][0])
            for (H, W), part in render.size_passes(sizes, frames_per_pass):
                masks = list(pool.map(lambda i: _load_mask(os.path.join(mask_folder, jobs[i][0] + ".npy"), (H, W)), part))
                for i, m in zip(part, masks):
                    if m is None:
                        print(f"Skipping {jobs[i][0]}: no {H} x {W} mask {os.path.join(mask_folder, jobs[i][0] + '.npy')}")
                        skipped.append(jobs[i][0])
                part = [i for i, m in zip(part, masks) if m is not None]
                masks = [m for m in masks if m is not None]
                if not part:
                    continue
                K = np.asarray(k_real, np.float64) if k_real is not None else render.default_camera(H, W, hamer.cfg)
                hands = [(n, h) for n, i in enumerate(part) for h in jobs[i][2]]
                first = np.cumsum([0] + [len(jobs[i][2]) for i in part])[:-1]          # a frame's first row of the mesh table
                meshes = []
                if hands:
                    verts = render.camera_vertices(hamer, [h for _, h in hands])
                    meshes = [{"frame": n, "vertices": verts[j], "faces": faces} for j, (n, _) in enumerate(hands)]
                mid = render.render_views(H, W, K, meshes, outputs=("mesh_id",), views=len(part), device=dev)["mesh_id"]
                gt = torch.from_numpy(np.stack(masks)).to(dev)
                queries = [(n, int(first[n]), int(first[n]) + len(jobs[i][2]), int(label)) for n, i in enumerate(part)]
                ev(mid, gt, queries, bound_th=bound_th)
                stems += [jobs[i][0] for i in part]
        per = ev.per_query()
        summary = ev.result() if ev.n else {"j_mean": float("nan"), "j_recall": float("nan"), "f_mean": float("nan"),
                                            "f_recall": float("nan"), "jf_mean": float("nan"), "n": 0}
    finally:
        render.release_workspaces()
        ME.release_workspaces()
    frames = {s: {k: float(per[k][n]) for k in ("J", "F", "precision", "recall")} for n, s in enumerate(stems)}
    result = {"frames": frames, **summary, "skipped": skipped, "n_skipped": len(skipped), "label": int(label),
              "bound_th": float(bound_th)}
    return result


def _contour_record(data: Dict, fitted: Dict) -> Dict:
    """The record with FIT_KEYS on every hand; ``fitted``: side -> (rotation (3, 3), cam_t, rms, pixels, applied) of the fitted
    hands.  An applied fit goes into ``pose_global`` (``evaluate_depth.fold_rotation``), ``theta[:3]`` where the record has one,
    and ``cam_t``; ``cam_t_unrefined`` and ``pose_global_unrefined`` keep what a depth refinement already put there.  A hand
    that was not moved keeps the bytes of every other key."""
    from .evaluate_depth import fold_rotation
    out = dict(data)
    for t in ("right", "left"):
        if data.get(t) is None:
            continue
        h = dict(data[t])
        old_t, old_g = h["cam_t"], h["pose_global"]
        h.setdefault("cam_t_unrefined", old_t)
        h.setdefault("pose_global_unrefined", old_g)
        h["mask_fit_rms_px"], h["mask_fit_pixels"], h["mask_fit"] = float("nan"), 0, False
        if t in fitted:
            R, cam_t, rms, pixels, applied = fitted[t]
            if applied:
                new = fold_rotation(old_g, R, bool(h["is_right"]))
                h["pose_global"] = new.astype(np.asarray(old_g).dtype).reshape(np.asarray(old_g).shape)
                if h.get("theta") is not None:
                    theta = np.array(h["theta"])
                    theta.reshape(-1)[:3] = h["pose_global"].reshape(-1)
                    h["theta"] = theta
                h["cam_t"] = np.asarray(cam_t, np.asarray(old_t).dtype).reshape(np.asarray(old_t).shape)
            h["mask_fit_rms_px"], h["mask_fit_pixels"], h["mask_fit"] = float(rms), int(pixels), bool(applied)
        out[t] = h
    return out


def refine_folder(image_folder, npy_folder, mask_folder, out_folder, hamer, k_real=None, label: int = 3, rounds: int = FIT_ROUNDS,
                  radius: Optional[int] = None, left_label: Optional[int] = None, rank: int = 0, world: int = 1,
                  frames_per_pass: int = FRAMES_PER_PASS, **fit_kw) -> Dict:
    """Write every record of ``npy_folder`` to ``out_folder`` (which may be the same folder) with its hands fitted to the label
    masks of ``mask_folder``: per pass of equally sized frames one MANO forward, one upload of the pass's masks and ONE
    ``fit_contour`` call about every hand's wrist joint (joint 0 of MANO, mirrored for a left hand, plus cam_t), folded into
    the records by ``_contour_record``.  A right hand is fitted to ``label``, a left hand to ``left_label`` (None: ``label``
    too); two hands under one label in one frame are fitted pred -> mask only (``fit_directions``).  ``k_real`` None: the
    camera the records were made with -- the scale-to-depth step is then consistent with that camera only; (3, 3) or
    {stem: (3, 3)}.  ``radius`` None: ``fit_radius(H, W)``; ``fit_kw`` goes to ``fit_contour``.  A record without a frame, a
    mask of the frame's size or a camera is written with the keys' defaults and named.  Returns ``{'records', 'hands',
    'fitted', 'skipped', 'n_skipped'}``.  The workspaces are released at the end."""
    import glob
    import torch
    from . import render
    from .hamer.utils import mask_eval as ME
    from .infer import _list_images, mano_hand_joints_vertices, shard_paths
    for v in (label, left_label):
        if v is not None and not 1 <= int(v) <= 255:
            raise ValueError(f"label must be in 1..255, got {v}")
    os.makedirs(out_folder, exist_ok=True)
    frames_by_stem = {os.path.splitext(os.path.basename(p))[0]: p for p in _list_images(image_folder)}
    jobs = []
    for npy in shard_paths(sorted(glob.glob(os.path.join(npy_folder, "*.npy"))), rank, world):
        stem = os.path.splitext(os.path.basename(npy))[0]
        data = np.load(npy, allow_pickle=True).item()
        jobs.append((stem, frames_by_stem.get(stem), data, [t for t in ("right", "left") if data.get(t) is not None]))
    dev = hamer.device
    faces = torch.as_tensor(np.asarray(hamer.mano.faces, np.int32), device=dev)
    fitted: Dict[int, Dict] = {}
    skipped = []
    n_hands = n_fitted = 0

    def skip(i, why):
        print(f"Skipping {jobs[i][0]}: {why}")
        skipped.append(jobs[i][0])

    def camera(stem, H, W):
        if k_real is None:
            return render.default_camera(H, W, hamer.cfg)
        k = k_real.get(stem) if isinstance(k_real, dict) else k_real
        return None if k is None else np.asarray(k, np.float64)

    try:
        with ThreadPoolExecutor(render._encode_threads()) as pool:
            usable = [i for i, j in enumerate(jobs) if j[3]]                     # a record without hands has nothing to move
            for i in [i for i in usable if jobs[i][1] is None]:
                skip(i, f"no frame in {image_folder}")
            usable = [i for i in usable if jobs[i][1] is not None]
            sizes = list(pool.map(render.frame_size, [jobs[i][1] for i in usable]))
            for i, hw in zip(usable, sizes):
                if hw is None:
                    skip(i, "image load failed")
            for (H, W), idx in render.size_passes(sizes, frames_per_pass):
                part = [usable[k] for k in idx]
                masks = list(pool.map(lambda i: _load_mask(os.path.join(mask_folder, jobs[i][0] + ".npy"), (H, W)), part))
                keep = []
                for n, i in enumerate(part):
                    if masks[n] is None:
                        skip(i, f"no {H} x {W} mask {os.path.join(mask_folder, jobs[i][0] + '.npy')}")
                    elif camera(jobs[i][0], H, W) is None:
                        skip(i, "no camera matrix")
                    else:
                        keep.append(n)
                if not keep:
                    continue
                part, masks = [part[n] for n in keep], [masks[n] for n in keep]
                K = np.stack([camera(jobs[i][0], H, W) for i in part])
                hands = [(n, i, t) for n, i in enumerate(part) for t in jobs[i][3]]
                recs = [jobs[i][2][t] for _, i, t in hands]
                sign = torch.tensor([[1.0, 1.0, 1.0] if h["is_right"] else [-1.0, 1.0, 1.0] for h in recs], device=dev)
                cam_t = torch.tensor(np.stack([np.asarray(h["cam_t"], np.float32).reshape(3) for h in recs]), device=dev)
                joints, verts = mano_hand_joints_vertices(hamer, recs)
                pivot = (joints[:, 0, :] * sign).to(torch.float64) + cam_t.to(torch.float64)
                labels = [int(label) if (t == "right" or left_label is None) else int(left_label) for _, _, t in hands]
                r = ME.fit_contour(H, W, K, verts * sign[:, None, :], faces, cam_t, pivot, [n for n, _, _ in hands],
                                   torch.from_numpy(np.stack(masks)).to(dev), labels, rounds=rounds, radius=radius, **fit_kw)
                rot, new, rms, pix, fit = (r[k].cpu().numpy() for k in ("rotation", "cam_t", "rms", "pixels", "fitted"))
                for j, (_, i, t) in enumerate(hands):
                    fitted.setdefault(i, {})[t] = (rot[j], new[j], rms[j], pix[j], fit[j])
                n_fitted += int(fit.sum())
        for i, job in enumerate(jobs):
            n_hands += len(job[3])
            np.save(os.path.join(out_folder, job[0] + ".npy"), _contour_record(job[2], fitted.get(i, {})))
    finally:
        render.release_workspaces()
        ME.release_fit_workspaces()
    return {"records": len(jobs), "hands": n_hands, "fitted": n_fitted, "skipped": skipped, "n_skipped": len(skipped)}


def format_line(result: Dict) -> str:
    return (f"{result['n']} frames: J mean {result['j_mean']:.4f} (recall {result['j_recall']:.4f}), F mean {result['f_mean']:.4f} "
            f"(recall {result['f_recall']:.4f}), J&F {result['jf_mean']:.4f}; label {result['label']}, bound_th {result['bound_th']:g}; "
            f"skipped {result['n_skipped']}")


def _parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description="score predicted hand meshes against label masks: region similarity J and contour accuracy F")
    ap.add_argument('--pred', type=str, required=True, help="folder of .npy hand records to score")
    ap.add_argument('--images', type=str, required=True, help="folder of the frames the records were made from (headers only: the size)")
    ap.add_argument('--masks', type=str, required=True, help="folder of <stem>.npy label images, --label on hand pixels")
    ap.add_argument('--label', type=int, default=3, help="the mask value of hand pixels (the reference's masks use 3)")
    ap.add_argument('--bound-th', type=float, default=0.008,
                    help="contour tolerance: a share of the image diagonal below 1, pixels from 1 up (at most 64 pixels)")
    ap.add_argument('--intrinsics', type=str, default=None, help="3x3 camera matrix txt the records were made with (default: the records' default camera)")
    ap.add_argument('--json', type=str, default=None, help="also write the result, per-frame scores included, to this file")
    ap.add_argument('--refine-to', type=str, default=None, metavar="DIR",
                    help="also write the records into DIR with every hand fitted to its mask: shift, scale (depth) and rotation "
                         "about the viewing axis, folded into cam_t and pose_global; prints J and F before and after")
    ap.add_argument('--fit-rounds', type=int, default=FIT_ROUNDS, help="with --refine-to: rounds of render, align and move (default 6)")
    ap.add_argument('--fit-radius', type=int, default=None, metavar="R",
                    help="with --refine-to: the search radius of the contour match in pixels, 0..64 (default: twice the tolerance "
                         "of the contour measure, 36 at 1080 x 1920)")
    ap.add_argument('--ckpt', type=str, default=None, help="hamer.ckpt path or synthetic:<seed> (default: config/hamer_config.py); only its MANO model is used")
    return ap


def main(argv=None):
    ap = _parser()
    args = ap.parse_args(argv)
    if not args.refine_to and (args.fit_rounds != FIT_ROUNDS or args.fit_radius is not None):
        ap.error("--fit-rounds / --fit-radius need --refine-to DIR")
    if args.fit_rounds < 0 or (args.fit_radius is not None and not 0 <= args.fit_radius <= 64):
        ap.error("--fit-rounds must not be negative and --fit-radius must be in 0..64")
    from .config.hamer_config import hamer_opt
    from .infer import hamer_inference, load_intrinsics
    if args.ckpt:
        hamer_opt.ckpt_path = args.ckpt
    k_real = load_intrinsics(args.intrinsics) if args.intrinsics else None
    hamer = hamer_inference(hamer_opt)
    result = score_folder(args.images, args.pred, args.masks, hamer, k_real, label=args.label, bound_th=args.bound_th)
    if args.refine_to:
        result["refine"] = refine_folder(args.images, args.pred, args.masks, args.refine_to, hamer, k_real, label=args.label,
                                         rounds=args.fit_rounds, radius=args.fit_radius)
        result["refined"] = score_folder(args.images, args.refine_to, args.masks, hamer, k_real, label=args.label, bound_th=args.bound_th)
        print(f"{result['refine']['fitted']} of {result['refine']['hands']} hands fitted into {args.refine_to}")
        print("before: " + format_line(result))
        print("after:  " + format_line(result["refined"]))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)
    print(format_line(result))
    for s in result["skipped"]:
        print(f"skipped: {s}")
    return result


if __name__ == '__main__':
    main()
