"""Measure how far the two hands of every two-hand record pass through each other, write it into the records, and move them apart.

    python -m hamer_yolo_amd.evaluate_penetration --pred <records dir> [--contact-tol-mm T] [--write-to DIR]
                                                  [--resolve-to DIR [--rounds N]] [--json out.json]

``--pred`` holds the ``<stem>.npy`` hand records the folder job writes.  HaMeR places each hand on its own, so the ``right`` and
the ``left`` mesh of one record can overlap in camera space.  For every record with both hands, every vertex of one hand gets its
signed distance to the surface of the other (negative inside), both ways: the interpenetration depth, the number of penetrating
vertices and the contact vertices (outside, within ``--contact-tol-mm``, default 2).  The MANO mesh is closed at the wrist for
this (``hamer.utils.penetration.close_boundaries``).  No images and no intrinsics are needed: the records' ``cam_t`` place the
hands.  The rule is in include/hamer_hip.h ("Penetration") and DESIGN.md section 10.7, with what the numbers do not say.

``--write-to DIR`` (which may be ``--pred``) writes every record again with, on both hands of a two-hand record,
``penetration_depth_m``, ``penetration_mean_m``, ``penetration_vertices``, ``contact_vertices``, ``vertices_signed_distance``
(778 float32) and ``vertices_contact`` (778 uint8 codes); a record with one hand or none is copied unchanged.

``--resolve-to DIR`` translates the two hands apart (``hamer.utils.penetration.resolve_penetration``, ``--rounds`` rounds) and
writes the records with ``cam_t`` moved, the keys above measured after the move, and ``cam_t_unresolved``,
``penetration_shift_m`` and ``penetration_resolved``.
"""
from __future__ import annotations

import argparse
import glob
import json
import os
from typing import Dict, List, Optional

import numpy as np

RECORDS_PER_PASS = 256
NEW_KEYS = ("penetration_depth_m", "penetration_mean_m", "penetration_vertices", "contact_vertices", "vertices_signed_distance",
            "vertices_contact")
RESOLVE_KEYS = ("cam_t_unresolved", "penetration_shift_m", "penetration_resolved")
SIDES = ("right", "left")


def _jobs(npy_folder, rank: int, world: int) -> List[tuple]:
    """(stem, record path, record, hand sides in right, left order) of this rank's share of the records."""
    from .infer import shard_paths
    jobs = []
    for npy in shard_paths(sorted(glob.glob(os.path.join(npy_folder, "*.npy"))), rank, world):
        data = np.load(npy, allow_pickle=True).item()
        jobs.append((os.path.splitext(os.path.basename(npy))[0], npy, data, [t for t in SIDES if data.get(t) is not None]))
    return jobs


def _scan(npy_folder, hamer, contact_tol_m, rank, world, records_per_pass, rounds: Optional[int] = None, gain=None):
    """The common loop of the three folder functions: (jobs, {job index: {side: per-hand results}}).  Per pass of two-hand
    records one MANO forward (``render.camera_vertices``) and one kernel call for both directions of every record -- or, with
    ``rounds``, the measure-then-move loop -- then one copy of each result to the host."""
    import torch
    from . import render
    from .hamer.utils import penetration as PN
    jobs = _jobs(npy_folder, rank, world)
    both = [i for i, j in enumerate(jobs) if len(j[3]) == 2]
    found: Dict[int, Dict] = {}
    faces = None
    try:
        for p0 in range(0, len(both), max(int(records_per_pass), 1)):
            part = both[p0:p0 + max(int(records_per_pass), 1)]
            verts = render.camera_vertices(hamer, [jobs[i][2][t] for i in part for t in SIDES])
            if faces is None:
                faces = torch.as_tensor(PN.closed_faces(hamer.mano.faces, int(verts.shape[1])), device=verts.device)
            meshes = [{"frame": k // 2, "vertices": verts[k], "faces": faces} for k in range(len(verts))]
            if rounds is None:
                r = PN.hand_penetration(meshes, contact_tol_m)
                shift = resolved = None
            else:
                kw = {} if gain is None else {"gain": gain}
                r = PN.resolve_penetration(meshes, PN.hand_pairs(meshes), rounds=rounds, contact_tol_m=contact_tol_m, **kw)
                shift, resolved = r["shift"].cpu().numpy(), r["resolved"].cpu().numpy()
            code, sd, sums = (r[k].cpu().numpy() for k in ("code", "signed_distance", "sums"))
            s, start = PN.summary(sums), r["row_start"]
            for q, (a, _) in enumerate(r["pairs"]):                       # query q: the vertices of mesh a, hand a % 2 of record a // 2
                f = {"codes": code[start[q]:start[q + 1]].copy(), "signed_distance": sd[start[q]:start[q + 1]].copy(),
                     **{k: s[k][q].item() for k in ("max_depth_m", "mean_depth_m", "inside", "contact", "tested", "status")}}
                if shift is not None:
                    f["shift"], f["resolved"] = shift[a].copy(), bool(resolved[a // 2])
                found.setdefault(part[a // 2], {})[SIDES[a % 2]] = f
    finally:
        PN.release_workspaces()
    return jobs, found


def _rows(jobs, found) -> List[Dict]:
    return [{"stem": job[0], "hand": t, **{k: found[i][t][k] for k in ("max_depth_m", "mean_depth_m", "inside", "contact", "tested", "status")}}
            for i, job in enumerate(jobs) if i in found for t in SIDES]


def score_folder(npy_folder, hamer, contact_tol_m: float = 0.002, rank: int = 0, world: int = 1,
                 records_per_pass: int = RECORDS_PER_PASS) -> Dict:
    """Interpenetration of every two-hand record of ``npy_folder``.  Returns ``{'rows': [{stem, hand, max_depth_m, mean_depth_m,
    inside, contact, tested, status}] (the hand's vertices against the other hand's surface), 'records', 'two_hand_records',
    'penetrating_records' (a vertex of either hand inside the other), 'max_depth_m' (the folder's largest, 0.0 without one),
    'mean_max_depth_m' (over the penetrating records, NaN without one)}``.  The workspace is released at the end."""
    jobs, found = _scan(npy_folder, hamer, contact_tol_m, rank, world, records_per_pass)
    rows = _rows(jobs, found)
    per_record = [max(found[i][t]["max_depth_m"] for t in SIDES) for i in sorted(found) if any(found[i][t]["inside"] for t in SIDES)]
    return {"rows": rows, "records": len(jobs), "two_hand_records": len(found), "penetrating_records": len(per_record),
            "max_depth_m": float(max(per_record)) if per_record else 0.0,
            "mean_max_depth_m": float(np.mean(per_record)) if per_record else float("nan")}


def annotated_record(data: Dict, found: Dict) -> Dict:
    """The record with NEW_KEYS on both hands (``found``: side -> the hand's results); every other key keeps its object."""
    out = dict(data)
    for t in SIDES:
        f, h = found[t], dict(data[t])
        h["penetration_depth_m"], h["penetration_mean_m"] = float(f["max_depth_m"]), float(f["mean_depth_m"])
        h["penetration_vertices"], h["contact_vertices"] = int(f["inside"]), int(f["contact"])
        h["vertices_signed_distance"] = np.asarray(f["signed_distance"], np.float32)
        h["vertices_contact"] = np.asarray(f["codes"], np.uint8)
        out[t] = h
    return out


def resolved_record(data: Dict, found: Dict) -> Dict:
    """``annotated_record`` (measured after the move) with ``cam_t`` moved by the hand's shift -- in ``cam_t``'s own dtype and
    shape -- and RESOLVE_KEYS: the ``cam_t`` the record came with, the shift in metres (3,) float32, and whether no vertex is
    inside afterwards."""
    out = annotated_record(data, found)
    for t in SIDES:
        h, cam_t = out[t], np.asarray(data[t]["cam_t"])
        shift = np.asarray(found[t]["shift"], np.float64)
        h["cam_t_unresolved"] = data[t]["cam_t"]
        h["cam_t"] = (cam_t.astype(np.float64) + shift.reshape(cam_t.shape)).astype(cam_t.dtype)
        h["penetration_shift_m"] = shift.astype(np.float32)
        h["penetration_resolved"] = bool(found[t]["resolved"])
    return out


def _write(jobs, found, out_folder, fold) -> None:
    os.makedirs(out_folder, exist_ok=True)
    for i, job in enumerate(jobs):
        dst = os.path.join(out_folder, job[0] + ".npy")
        if i in found:
            np.save(dst, fold(job[2], found[i]))
        elif os.path.abspath(dst) != os.path.abspath(job[1]):
            with open(job[1], "rb") as src, open(dst, "wb") as out:
                out.write(src.read())


def annotate_folder(npy_folder, out_folder, hamer, contact_tol_m: float = 0.002, rank: int = 0, world: int = 1,
                    records_per_pass: int = RECORDS_PER_PASS) -> Dict:
    """Write every record of ``npy_folder`` to ``out_folder`` (which may be the same folder) with NEW_KEYS on both hands of
    every two-hand record: ``penetration_depth_m`` and ``penetration_mean_m`` (floats: the largest and the mean depth of the
    hand's vertices inside the other hand, 0.0 without one), ``penetration_vertices`` and ``contact_vertices`` (ints),
    ``vertices_signed_distance`` (778,) float32 and ``vertices_contact`` (778,) uint8 (``hamer.utils.penetration.CODES``).  Every
    other record is copied unchanged.  Returns ``{'records', 'annotated' (records), 'penetrating' (records)}``."""
    jobs, found = _scan(npy_folder, hamer, contact_tol_m, rank, world, records_per_pass)
    _write(jobs, found, out_folder, annotated_record)
    return {"records": len(jobs), "annotated": len(found), "penetrating": sum(any(f[t]["inside"] for t in SIDES) for f in found.values())}


def resolve_folder(npy_folder, out_folder, hamer, contact_tol_m: float = 0.002, rounds: int = 8, gain=None, rank: int = 0,
                   world: int = 1, records_per_pass: int = RECORDS_PER_PASS) -> Dict:
    """``annotate_folder`` after moving the two hands of every two-hand record apart (``resolve_penetration``: ``rounds``
    rounds, translations only): ``cam_t`` becomes ``cam_t + shift``, NEW_KEYS hold the measurement after the move, and
    RESOLVE_KEYS are added.  Returns ``{'records', 'annotated', 'moved' (records with a shift), 'unresolved' (records with a
    vertex still inside)}``."""
    jobs, found = _scan(npy_folder, hamer, contact_tol_m, rank, world, records_per_pass, rounds=int(rounds), gain=gain)
    _write(jobs, found, out_folder, resolved_record)
    return {"records": len(jobs), "annotated": len(found), "moved": sum(any(np.any(f[t]["shift"] != 0) for t in SIDES) for f in found.values()),
            "unresolved": sum(not f["right"]["resolved"] for f in found.values())}


def format_line(result: Dict) -> str:
    return (f"{result['two_hand_records']} two-hand records of {result['records']}: {result['penetrating_records']} interpenetrate, "
            f"deepest {result['max_depth_m'] * 1e3:.2f} mm, mean of the records' deepest {result['mean_max_depth_m'] * 1e3:.2f} mm")


def _parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description="measure and resolve the interpenetration of the two hands of every two-hand record")
    ap.add_argument('--pred', type=str, required=True, help="folder of .npy hand records")
    ap.add_argument('--contact-tol-mm', type=float, default=2.0, metavar="T",
                    help="a vertex outside the other hand and within T millimetres of it is a contact vertex (default 2)")
    ap.add_argument('--write-to', type=str, default=None, metavar="DIR", help="also write the records with the penetration keys into DIR")
    ap.add_argument('--resolve-to', type=str, default=None, metavar="DIR",
                    help="also move the hands of every two-hand record apart and write the records, cam_t moved, into DIR")
    ap.add_argument('--rounds', type=int, default=8, metavar="N", help="with --resolve-to: measure-then-move rounds (default 8)")
    ap.add_argument('--json', type=str, default=None, help="also write the result, per-hand rows included, to this file")
    ap.add_argument('--ckpt', type=str, default=None, help="hamer.ckpt path or synthetic:<seed> (default: config/hamer_config.py); only its MANO model is used")
    return ap


def main(argv=None):
    ap = _parser()
    args = ap.parse_args(argv)
    if not (np.isfinite(args.contact_tol_mm) and 0.0 <= args.contact_tol_mm <= 1000.0):
        ap.error("--contact-tol-mm must lie in 0 .. 1000")
    if args.rounds != 8 and not args.resolve_to:
        ap.error("--rounds needs --resolve-to DIR")
    if args.rounds < 0:
        ap.error("--rounds must be >= 0")
    from .config.hamer_config import hamer_opt
    from .infer import hamer_inference
    if args.ckpt:
        hamer_opt.ckpt_path = args.ckpt
    hamer = hamer_inference(hamer_opt)
    tol = args.contact_tol_mm * 1e-3
    result = score_folder(args.pred, hamer, tol)
    if args.write_to:
        result["annotate"] = annotate_folder(args.pred, args.write_to, hamer, tol)
        print(f"{result['annotate']['annotated']} two-hand records annotated into {args.write_to}")
    if args.resolve_to:
        result["resolve"] = resolve_folder(args.pred, args.resolve_to, hamer, tol, rounds=args.rounds)
        print(f"{result['resolve']['moved']} records moved apart into {args.resolve_to}, {result['resolve']['unresolved']} still interpenetrate")
    if args.json:
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)
    print(format_line(result))
    return result


if __name__ == '__main__':
    main()
