"""Compare two folders of the drivers' ``.npy`` records in the field's hand metrics, in millimetres.

    python -m hamer_yolo_amd.evaluate --pred A --ref B [--json out.json] [--mesh-scores]

Both folders hold what ``process_batch_manopara`` writes (``{'left': None | hand, 'right': None | hand}`` per image, a hand
being ``betas``, ``pose_global``, ``pose_hand``, ``cam_t``, ``is_right``); a ground-truth folder in the same format works too.
Hands are paired by file stem and side.  Every paired hand is rebuilt by MANO (one forward per folder), left hands mirrored
as ``reconstruct_and_save_obj_with_wrapper`` does; its 21 joints and 778 vertices form one [799][3] point set and two
``hm_pose_eval`` launches score all pairs: the joints (MPJPE / PA-MPJPE, wrist-relative) and the vertices (MPVPE / PA-MPVPE,
wrist-relative).  ``cam_t`` is NOT added to the points: all four metrics are relative to the wrist, where a translation
cancels exactly, and adding it in fp32 would first round every coordinate at the magnitude of the depth (2.4e-7 m at 2 m, the
order of the distances between two precision routes).  The translation is reported on its own, as ``root``, from the records.

``--mesh-scores`` (``compare_folders_with(..., mesh_scores=True)``) adds the other half of the field's tables: F@5 mm and F@15 mm
of the 778 vertices and the area under the PCK curve over 0-50 mm of joints and vertices, each raw and Procrustes-aligned
(``hamer.utils.mesh_eval.MeshEvaluator``: hm_mesh_score, hm_pck_auc).  The points are the same wrist-relative ones: FreiHAND's
UNALIGNED F-score is taken on absolute coordinates, this driver's is not (cam_t is not added, see above), so only the aligned
F-scores and the AUCs compare with published tables.  The F-score rule is unpinned against FreiHAND's script.
"""
from __future__ import annotations

import argparse
import glob
import json
import os
from typing import Dict, List, Optional, Tuple

import numpy as np

SIDES = ("right", "left")
N_JOINTS = 21
STATS = ("mean", "median", "p95", "max")
METRICS = ("mpjpe", "pa_mpjpe", "mpvpe", "pa_mpvpe", "root", "max_dtheta", "max_dbeta")


def _load_folder(folder: str) -> Dict[Tuple[str, str], Dict]:
    hands = {}
    for path in sorted(glob.glob(os.path.join(folder, "*.npy"))):
        stem = os.path.splitext(os.path.basename(path))[0]
        data = np.load(path, allow_pickle=True).item()
        for side in SIDES:
            if data.get(side) is not None:
                hands[(stem, side)] = data[side]
    return hands


def pair_records(pred_dir: str, ref_dir: str):
    """-> (pairs, only_pred, only_ref): pairs is a list of (stem, side, pred hand, ref hand) in (stem, side) order; the other
    two list the (stem, side) present in one folder only (a missing file, or a hand missing from a file).  No GPU."""
    pred, ref = _load_folder(pred_dir), _load_folder(ref_dir)
    pairs = [(k[0], k[1], pred[k], ref[k]) for k in sorted(pred) if k in ref]
    return pairs, [k for k in sorted(pred) if k not in ref], [k for k in sorted(ref) if k not in pred]


def summary(values) -> Dict[str, float]:
    """mean / median / p95 / max of a per-hand vector."""
    v = np.asarray(values, np.float64)
    if v.size == 0:
        return {k: float("nan") for k in STATS}
    return {"mean": float(v.mean()), "median": float(np.median(v)), "p95": float(np.percentile(v, 95)), "max": float(v.max())}


def _hand_points(hamer, hands: List[Dict]):
    """(B, 799, 3) on the device: joints then vertices in the hand's own frame, left hands mirrored (no cam_t: module docstring)."""
    import torch
    from .infer import mano_hand_joints_vertices
    joints, verts = mano_hand_joints_vertices(hamer, hands)
    pts = torch.cat([joints, verts], 1)
    sign = torch.tensor([[1.0 if hd['is_right'] else -1.0, 1.0, 1.0] for hd in hands], device=pts.device)
    return (pts * sign[:, None, :]).contiguous()


def compare_folders(pred_dir: str, ref_dir: str, hamer, json_path: Optional[str] = None) -> Dict:
    """Score the hands of ``pred_dir`` against those of ``ref_dir``.  Returns ``{'pairs', 'only_pred', 'only_ref' (counts),
    'only_pred_hands', 'only_ref_hands', 'hands' (lists of "stem/side"), 'metrics': {name: {mean, median, p95, max}},
    'per_hand': {name: [...]}}``; distances in mm, ``max_dtheta`` in radians, ``max_dbeta`` in MANO shape units."""
    return compare_folders_with(pred_dir, ref_dir, hamer, json_path)


def compare_folders_with(pred_dir: str, ref_dir: str, hamer, json_path: Optional[str] = None, mesh_scores: bool = False) -> Dict:
    """``compare_folders`` with its opt-in parts.  ``mesh_scores=True`` adds ONE key to the result, ``'mesh_scores'``:
    ``{'per_hand': {f5, f15, pa_f5, pa_f15: [...]}, 'metrics': {name: {mean, median, p95, max}}, 'auc': {auc_j, auc_v,
    pa_auc_j, pa_auc_v, val_min, val_max, steps}}`` -- F-scores of the vertices at 5 and 15 mm and areas under the 0-50 mm PCK
    curves of joints and vertices, raw (wrist-relative, NOT FreiHAND's absolute coordinates) and Procrustes-aligned.
    Everything else in the result is what ``compare_folders`` returns."""
    import torch
    from .hamer.utils.pose_utils import pose_eval
    pairs, only_pred, only_ref = pair_records(pred_dir, ref_dir)
    per_hand: Dict[str, np.ndarray] = {m: np.zeros(0) for m in METRICS}
    if pairs:
        P = _hand_points(hamer, [p[2] for p in pairs])
        G = _hand_points(hamer, [p[3] for p in pairs])
        n_pts = P.shape[1]
        j = pose_eval(P, G, root=0, sel=range(N_JOINTS))
        v = pose_eval(P, G, root=0, sel=range(N_JOINTS, n_pts))
        mm = (torch.stack([j["err"], j["pa_err"], v["err"], v["pa_err"]]).double() * 1000.0).cpu().numpy()      # the one copy
        for name, row in zip(METRICS[:4], mm):
            per_hand[name] = row
        f64 = lambda hd, k: np.asarray(hd[k], np.float64).reshape(-1)                                            # noqa: E731
        per_hand["root"] = np.array([1000.0 * np.linalg.norm(f64(a, 'cam_t') - f64(b, 'cam_t')) for _, _, a, b in pairs])
        theta = lambda hd: np.concatenate([f64(hd, 'pose_global'), f64(hd, 'pose_hand')])                        # noqa: E731
        per_hand["max_dtheta"] = np.array([np.abs(theta(a) - theta(b)).max() for _, _, a, b in pairs])
        per_hand["max_dbeta"] = np.array([np.abs(f64(a, 'betas') - f64(b, 'betas')).max() for _, _, a, b in pairs])
    name = lambda k: f"{k[0]}/{k[1]}"                                                                            # noqa: E731
    result = {"pairs": len(pairs), "only_pred": len(only_pred), "only_ref": len(only_ref),
              "only_pred_hands": [name(k) for k in only_pred], "only_ref_hands": [name(k) for k in only_ref],
              "hands": [name(p[:2]) for p in pairs],
              "metrics": {m: summary(per_hand[m]) for m in METRICS},
              "per_hand": {m: [float(x) for x in per_hand[m]] for m in METRICS}}
    if mesh_scores:
        from .hamer.utils.mesh_eval import MeshEvaluator
        ev = MeshEvaluator(max(len(pairs), 1), N_JOINTS, root=0)
        auc = {k: float("nan") for k in ("auc_j", "auc_v", "pa_auc_j", "pa_auc_v")}
        if pairs:
            ev(P, G)
            auc = {k: v for k, v in ev.result().items() if k in auc}
        f = ev.per_hand()
        auc.update({"val_min": ev.auc[0], "val_max": ev.auc[1], "steps": ev.auc[2]})
        result["mesh_scores"] = {"per_hand": {k: [float(x) for x in f[k]] for k in ev.f_names},
                                 "metrics": {k: summary(f[k]) for k in ev.f_names}, "auc": auc}
    if json_path:
        with open(json_path, "w") as f:
            json.dump(result, f, indent=1)
    return result


def format_line(result: Dict) -> str:
    m = result["metrics"]
    head = " ".join(f"{k} {m[k]['mean']:.4f}" for k in ("mpjpe", "pa_mpjpe", "mpvpe", "pa_mpvpe"))
    return (f"{result['pairs']} hands: {head} mm (mean; max {m['mpvpe']['max']:.4f}), root {m['root']['mean']:.4f} mm, "
            f"max |dtheta| {m['max_dtheta']['max']:.3g}, max |dbeta| {m['max_dbeta']['max']:.3g}; "
            f"only in pred {result['only_pred']}, only in ref {result['only_ref']}")


def format_mesh_line(result: Dict) -> str:
    """The line ``--mesh-scores`` adds: mean F-scores of the vertices and the areas under the PCK curves."""
    ms = result["mesh_scores"]
    f = " ".join(f"{'PA-' if k.startswith('pa_') else ''}F@{k.split('f')[-1]} {v['mean']:.4f}" for k, v in ms["metrics"].items())
    a = ms["auc"]
    auc = " ".join(f"{n} {a[k]:.4f}" for k, n in (("auc_j", "J"), ("auc_v", "V"), ("pa_auc_j", "PA-J"), ("pa_auc_v", "PA-V")))
    return (f"mesh scores (wrist-relative): {f} (mean); AUC {1000 * a['val_min']:g}-{1000 * a['val_max']:g} mm, "
            f"{a['steps']} steps: {auc}")


def _parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description="compare two folders of hand records: MPJPE / PA-MPJPE / MPVPE / PA-MPVPE in mm")
    ap.add_argument('--pred', type=str, required=True, help="folder of .npy records to score")
    ap.add_argument('--ref', type=str, required=True, help="folder of .npy records to score against (another route, or ground truth)")
    ap.add_argument('--json', type=str, default=None, help="also write the full result, per-hand vectors included, to this file")
    ap.add_argument('--mesh-scores', action='store_true',
                    help="also report F@5 / F@15 of the vertices and the AUC of the 0-50 mm PCK curves, raw and Procrustes-aligned")
    ap.add_argument('--ckpt', type=str, default=None, help="hamer.ckpt path or synthetic:<seed> (default: config/hamer_config.py); only its MANO model is used")
    return ap


def main(argv=None):
    args = _parser().parse_args(argv)
    from .config.hamer_config import hamer_opt
    from .infer import hamer_inference
    if args.ckpt:
        hamer_opt.ckpt_path = args.ckpt
    result = compare_folders_with(args.pred, args.ref, hamer_inference(hamer_opt), args.json, mesh_scores=args.mesh_scores)
    print(format_line(result))
    if args.mesh_scores:
        print(format_mesh_line(result))
    return result


if __name__ == '__main__':
    main()
