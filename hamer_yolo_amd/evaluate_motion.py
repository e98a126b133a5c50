"""Measure the frame-to-frame jitter of the hand tracks of a folder of records, and smooth them.

    python -m hamer_yolo_amd.evaluate_motion --pred <records dir> [--fps F] [--smooth-to DIR [--radius R] [--sigma S] [--max-fill K]]
                                             [--json out.json] [--ckpt ...]

``--pred`` holds the ``<stem>.npy`` hand records the folder job writes, one per frame of a video; the stems are ordered with runs
of digits as integers (``frame_2`` before ``frame_10``).  A track is one side, right or left, over the frames.  Reported per
side and overall: the acceleration |x[t-1] - 2 x[t] + x[t+1]|, averaged over the points, of the 21 joints in the camera frame,
of the joints relative to the wrist, and of the 778 vertices, in mm per frame^2 (with ``--fps`` also m/s^2), wherever three
frames in a row hold the hand.  No images and no intrinsics are needed.  The rule is in include/hamer_hip.h ("Motion") and
DESIGN.md section 10.8, with what the numbers do not say.

``--smooth-to DIR`` (which may be ``--pred``) writes every record again, smoothed over time (``hamer.utils.motion``): a zero-phase
window of ``--radius`` frames each way (default 4) with Gaussian weights of ``--sigma`` frames (default 2), rotations averaged as
rotations.  A smoothed hand gets new ``pose_global``, ``pose_hand``, ``theta``, ``betas`` and ``cam_t`` and keeps the old ones as
``*_unsmoothed``, with ``track_status``, ``track_pairs`` and ``track_moved_deg``; a missing hand whose neighbours at most
``--max-fill`` frames away (default 2; 0: never) are present on both sides is filled and flagged ``track_filled``.
"""
from __future__ import annotations

import argparse
import glob
import json
import os
from typing import Dict, List

import numpy as np

RECORDS_PER_PASS = 256
SIDES = ("right", "left")
POINT_SETS = ("joints", "joints_rel", "vertices")


def load_sequence(npy_folder) -> List[tuple]:
    """(stem, path, record) of every record of the folder, in ``natural_key`` order."""
    from .hamer.utils.motion import natural_key
    paths = glob.glob(os.path.join(npy_folder, "*.npy"))
    stems = {p: os.path.splitext(os.path.basename(p))[0] for p in paths}
    return [(stems[p], p, np.load(p, allow_pickle=True).item()) for p in sorted(paths, key=lambda p: natural_key(stems[p]))]


def score_records(records: List[dict], hamer, fps=None, records_per_pass: int = RECORDS_PER_PASS) -> Dict:
    """The three accelerations of a sorted sequence of records: the MANO forward in passes (``render.camera_joints_vertices``),
    three ``track_jitter`` calls, one copy each to the host.  Returns ``{point set: {'right', 'left', 'all': summary}}`` and
    ``'accel'``: the (N, 2) arrays in metres per frame^2."""
    import torch
    from . import render
    from .hamer.utils import motion as MO
    N = len(records)
    dev = hamer.device
    hands = [(t, s) for t, rec in enumerate(records) for s, side in enumerate(SIDES) if rec.get(side) is not None]
    joints = torch.zeros(N, 2, 21, 3, dtype=torch.float64, device=dev)
    verts = torch.zeros(N, 2, 778, 3, dtype=torch.float64, device=dev)
    present = torch.zeros(N, 2, dtype=torch.uint8, device=dev)
    step = max(int(records_per_pass), 1)
    for p0 in range(0, len(hands), step):
        part = hands[p0:p0 + step]
        j, v = render.camera_joints_vertices(hamer, [records[t][SIDES[s]] for t, s in part])
        ti = torch.tensor([t for t, _ in part], device=dev)
        si = torch.tensor([s for _, s in part], device=dev)
        joints[ti, si] = j.to(torch.float64)
        verts[ti, si] = v.to(torch.float64)[:, :778]
        present[ti, si] = 1
    sets = {"joints": joints, "joints_rel": joints - joints[:, :, :1], "vertices": verts}
    out: Dict = {"accel": {}}
    for name in POINT_SETS:
        a = MO.track_jitter(sets[name], present).cpu().numpy() if N else np.zeros((0, 2))
        out["accel"][name] = a
        out[name] = {"right": MO.summary(a[:, 0], fps), "left": MO.summary(a[:, 1], fps), "all": MO.summary(a, fps)}
    return out


def score_folder(npy_folder, hamer, fps=None, records_per_pass: int = RECORDS_PER_PASS) -> Dict:
    """Jitter of the tracks of ``npy_folder``: ``{'records', 'hands', 'joints', 'joints_rel', 'vertices'}``, each point set as
    ``{'right', 'left', 'all'}`` of ``hamer.utils.motion.summary`` (mm per frame^2; ``n`` frames with both neighbours)."""
    seq = load_sequence(npy_folder)
    r = score_records([rec for _, _, rec in seq], hamer, fps, records_per_pass)
    r.pop("accel")
    r["records"] = len(seq)
    r["hands"] = sum(rec.get(t) is not None for _, _, rec in seq for t in SIDES)
    return r


def smooth_folder(npy_folder, out_folder, hamer, radius: int = 4, sigma: float = 2.0, max_fill: int = 2) -> Dict:
    """Write every record of ``npy_folder`` to ``out_folder`` (which may be the same folder), smoothed over the whole sequence
    (``hamer.utils.motion.smooth_hands``).  Returns ``{'records', 'smoothed', 'filled', 'kept', 'degenerate' (hands),
    'max_moved_deg', 'max_moved_stem'}``: the largest rotation any joint of a smoothed hand was moved by, and its record."""
    from .hamer.utils import motion as MO
    seq = load_sequence(npy_folder)
    new = MO.smooth_hands(hamer, [rec for _, _, rec in seq], radius, sigma, max_fill)
    os.makedirs(out_folder, exist_ok=True)
    count = {"SMOOTHED": 0, "FILLED": 0, "KEPT": 0, "DEGENERATE": 0}
    worst, worst_stem = 0.0, None
    for (stem, _, _), rec in zip(seq, new):
        for t in SIDES:
            h = rec.get(t)
            if h is None:
                continue
            count[h["track_status"]] += 1
            if "track_moved_deg" in h and float(np.max(h["track_moved_deg"])) > worst:
                worst, worst_stem = float(np.max(h["track_moved_deg"])), stem
        np.save(os.path.join(out_folder, stem + ".npy"), rec)
    return {"records": len(seq), "smoothed": count["SMOOTHED"], "filled": count["FILLED"], "kept": count["KEPT"],
            "degenerate": count["DEGENERATE"], "max_moved_deg": worst, "max_moved_stem": worst_stem}


def format_line(result: Dict) -> str:
    unit = "mm/frame^2"
    line = (f"{result['hands']} hands in {result['records']} records: mean acceleration joints {result['joints']['all']['mean']:.3f}, "
            f"wrist-relative {result['joints_rel']['all']['mean']:.3f}, vertices {result['vertices']['all']['mean']:.3f} {unit}")
    if "after" in result:
        a, s = result["after"], result["smooth"]
        line += (f"; smoothed: joints {a['joints']['all']['mean']:.3f}, wrist-relative {a['joints_rel']['all']['mean']:.3f}, vertices "
                 f"{a['vertices']['all']['mean']:.3f} {unit}; {s['smoothed']} hands smoothed, {s['filled']} filled, {s['kept']} kept, "
                 f"{s['degenerate']} degenerate; largest joint rotation {s['max_moved_deg']:.2f} deg ({s['max_moved_stem']})")
    return line


def _parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description="measure and smooth the frame-to-frame jitter of the hand tracks of a folder of records")
    ap.add_argument('--pred', type=str, required=True, help="folder of .npy hand records, one per frame")
    ap.add_argument('--fps', type=float, default=None, metavar="F", help="also report the accelerations in m/s^2 at F frames per second")
    ap.add_argument('--smooth-to', type=str, default=None, metavar="DIR", help="also write the records, smoothed over time, into DIR")
    ap.add_argument('--radius', type=int, default=None, metavar="R", help="with --smooth-to: frames each way, 0..32 (default 4)")
    ap.add_argument('--sigma', type=float, default=None, metavar="S", help="with --smooth-to: the Gaussian window's sigma in frames (default 2)")
    ap.add_argument('--max-fill', type=int, default=None, metavar="K",
                    help="with --smooth-to: fill a missing hand only from a pair of neighbours at most K frames away (default 2; 0: never)")
    ap.add_argument('--json', type=str, default=None, help="also write the result to this file")
    ap.add_argument('--ckpt', type=str, default=None, help="hamer.ckpt path or synthetic:<seed> (default: config/hamer_config.py); only its MANO model is used")
    return ap


def smooth_options(ap: argparse.ArgumentParser, on: bool, flag: str, names: Dict[str, str], radius, sigma, max_fill) -> tuple:
    """Usage errors of a radius / sigma / max-fill triple that needs the switch ``flag``; (radius, sigma, max_fill) with the
    defaults filled in.  ``names``: the option names for the messages."""
    from .hamer.utils.motion import MAX_FILL, MAX_RADIUS, RADIUS, SIGMA
    given = [names[k] for k, v in (("radius", radius), ("sigma", sigma), ("max_fill", max_fill)) if v is not None]
    if given and not on:
        ap.error(f"{' / '.join(given)} need{'s' if len(given) == 1 else ''} {flag}")
    if radius is not None and not 0 <= radius <= MAX_RADIUS:
        ap.error(f"{names['radius']} must be in 0..{MAX_RADIUS}")
    if sigma is not None and not (np.isfinite(sigma) and sigma > 0):
        ap.error(f"{names['sigma']} must be > 0")
    if max_fill is not None and max_fill < 0:
        ap.error(f"{names['max_fill']} must be >= 0")
    return (RADIUS if radius is None else radius, SIGMA if sigma is None else sigma, MAX_FILL if max_fill is None else max_fill)


def main(argv=None):
    ap = _parser()
    args = ap.parse_args(argv)
    if args.fps is not None and not (np.isfinite(args.fps) and args.fps > 0):
        ap.error("--fps must be > 0")
    radius, sigma, max_fill = smooth_options(ap, bool(args.smooth_to), "--smooth-to DIR",
                                             {"radius": "--radius", "sigma": "--sigma", "max_fill": "--max-fill"},
                                             args.radius, args.sigma, args.max_fill)
    from .config.hamer_config import hamer_opt
    from .infer import hamer_inference
    if args.ckpt:
        hamer_opt.ckpt_path = args.ckpt
    hamer = hamer_inference(hamer_opt)
    result = score_folder(args.pred, hamer, args.fps)
    if args.smooth_to:
        result["smooth"] = smooth_folder(args.pred, args.smooth_to, hamer, radius, sigma, max_fill)
        result["after"] = score_folder(args.smooth_to, hamer, args.fps)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)
    print(format_line(result))
    return result


if __name__ == '__main__':
    main()
