"""Score predicted hand meshes against per-frame label masks: region similarity J and contour accuracy F.

    python -m hamer_yolo_amd.evaluate_masks --pred <records dir> --images <frames dir> --masks <mask dir>
                                            [--label 3] [--bound-th 0.008] [--intrinsics K.txt] [--json out.json]

``--pred`` holds the ``<stem>.npy`` hand records the folder job writes, ``--images`` the frames they were made from (only
their headers are read, for the size) and ``--masks`` one ``<stem>.npy`` label image per frame, ``--label`` on hand pixels:
the masks ``process_batch_manopara_with_mask`` / ``get_bbox_from_npy`` read and ``--hand-maps`` writes.  Per frame the
silhouette of ALL its predicted hands (the z-buffered renderer's coverage) is scored against the pixels that carry the label,
because such masks carry one hand label and do not tell the hands apart.  Masks with a label per hand can be scored per hand
through ``hamer.utils.mask_eval.mask_counts`` with one query per hand.

J is intersection over union; F is the harmonic mean of boundary precision and recall within ``bound_th`` of the image
diagonal (``bound_radius``: 18 pixels at 1080 x 1920).  The rule is the DAVIS benchmark's J and F written from their
definition (include/hamer_hip.h); it is unpinned against DAVIS's own script.

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
    ap.add_argument('--ckpt', type=str, default=None, help="hamer.ckpt path or synthetic:<seed> (default: config/hamer_config.py); only its MANO model is used")
    return ap


def main(argv=None):
    args = _parser().parse_args(argv)
    from .config.hamer_config import hamer_opt
    from .infer import hamer_inference, load_intrinsics
    if args.ckpt:
        hamer_opt.ckpt_path = args.ckpt
    k_real = load_intrinsics(args.intrinsics) if args.intrinsics else None
    result = score_folder(args.images, args.pred, args.masks, hamer_inference(hamer_opt), k_real, label=args.label,
                          bound_th=args.bound_th)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)
    print(format_line(result))
    for s in result["skipped"]:
        print(f"skipped: {s}")
    return result


if __name__ == '__main__':
    main()
