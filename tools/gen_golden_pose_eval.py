#!/usr/bin/env python3
"""Generate tests/golden/pose_eval.npz from the REFERENCE's hamer/hamer/utils/pose_utils.py (loaded by file path from the
reference tree: the package beside it imports pyrender; the module itself needs torch and numpy only; CPU).

Per case: the fp32 inputs, the reference's fp32 ``compute_similarity_transform``, ``reconstruction_error`` and ``eval_pose``,
and ``ref32_dist`` per quantity -- the largest distance, over the case's hands, between the reference's fp32 output and the
fp64 rule (tests/pose_eval_rule.py) on the same inputs.  One ``Evaluator`` pass (two batches, 4 + 3), and the parameter names of the public callables.

Every stored case outside the exempt ones (N = 2, planar) meets the conditioning rule on K's singular values, by the sign of
det(U V^T):  +1: (s2 + s3) / s1 >= 0.05;  -1: (s2 - s3) / s1 >= 0.05  -- so that R is well conditioned and the reference's fp32
answer means something.  The seed of a case is the first for which every hand meets it.  Data only, no code."""
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pose_eval_rule as PR  # noqa: E402
from tools.gen_golden_rootnet import REF  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "pose_eval.npz")
B = 7
SIZES = (3, 21, 64, 65, 778, 1024)
KEYPOINT_LIST = [0, 2, 3, 5, 8, 9, 12, 13, 17, 20]
PELVIS = 9
COND = 0.05


def load_reference():
    spec = importlib.util.spec_from_file_location("ref_pose_utils", os.path.join(REF, "hamer", "hamer", "utils", "pose_utils.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def well_conditioned(pred, gt):
    _, _, _, _, sign, s = PR.similarity_transform(pred, gt)
    margin = np.where(sign > 0, (s[:, 1] + s[:, 2]) / s[:, 0], (s[:, 1] - s[:, 2]) / s[:, 0])
    return bool((margin >= COND).all())


def rotation(rng):
    q = rng.normal(size=4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def hand_sets(rng, n):
    """B hand-sized point sets (metres): a cloud of 8 cm around a point half a metre away, and a noisy, shifted prediction."""
    gt = rng.normal(size=(B, n, 3)) * 0.04 + rng.normal(size=(B, 1, 3)) * 0.1 + np.array([0.0, 0.0, 0.5])
    pred = gt + rng.normal(size=(B, n, 3)) * 0.008 + rng.normal(size=(B, 1, 3)) * 0.02
    return pred.astype(np.float32), gt.astype(np.float32)


def case_random(seed, n):
    return hand_sets(np.random.default_rng(seed), n)


def case_similarity(seed):
    rng = np.random.default_rng(seed)
    pred = rng.normal(size=(B, 21, 3)) * 0.04
    gt = np.stack([2.5 * pred[b] @ rotation(rng).T + rng.normal(size=3) * 0.3 for b in range(B)])
    return pred.astype(np.float32), gt.astype(np.float32)


def case_mirror(seed):
    rng = np.random.default_rng(seed)
    pred = (rng.normal(size=(B, 21, 3)) * np.array([0.05, 0.03, 0.015])).astype(np.float32)
    return pred, pred * np.array([-1.0, 1.0, 1.0], np.float32)


def case_planar_mirror(seed):
    rng = np.random.default_rng(seed)
    pred = (rng.normal(size=(B, 21, 3)) * 0.05).astype(np.float32)
    pred[:, :, 2] = np.float32(0.25)                                     # the plane z = 0.25, exactly
    return pred, pred * np.array([-1.0, 1.0, 1.0], np.float32)           # a half turn about the y axis through the centroid fits


def first_seed(make, start, exempt=False):
    for seed in range(start, start + 1000):
        pred, gt = make(seed)
        if exempt or well_conditioned(pred, gt):
            return seed, pred, gt
    raise RuntimeError("no seed meets the conditioning rule")


def main():
    ref = load_reference()
    out = {"keypoint_list": np.array(KEYPOINT_LIST, np.int64), "pelvis_ind": np.int64(PELVIS), "cond": np.float64(COND)}
    cases = [(f"rand{n}", (lambda s, n=n: case_random(s, n)), 100 + n, False) for n in SIZES]
    cases += [("similarity", case_similarity, 2000, False), ("mirror", case_mirror, 3000, False),
              ("identical", lambda s: (case_random(s, 21)[1],) * 2, 4000, False),
              ("planar_mirror", case_planar_mirror, 5000, True), ("two", lambda s: case_random(s, 2), 6000, True)]
    names, exempt_names = [], []
    for name, make, start, exempt in cases:
        seed, pred, gt = first_seed(make, start, exempt)
        tp, tg = torch.from_numpy(pred), torch.from_numpy(gt)
        hat = ref.compute_similarity_transform(tp, tg).numpy()
        re = ref.reconstruction_error(tp, tg).numpy()
        mpjpe_mm, re_mm = ref.eval_pose(tp, tg)
        rule = PR.pose_eval(pred, gt)
        out.update({f"{name}/pred": pred, f"{name}/gt": gt, f"{name}/seed": np.int64(seed), f"{name}/ref_s1hat": hat,
                    f"{name}/ref_re": re, f"{name}/ref_mpjpe_mm": mpjpe_mm, f"{name}/ref_re_mm": re_mm})
        if not exempt:
            dist = {"s1hat": np.abs(hat - rule["aligned"]).max(), "err": np.abs(mpjpe_mm / np.float32(1000) - rule["err"]).max(),
                    "pa_err": np.abs(re - rule["pa_err"]).max(), "err_mm": np.abs(mpjpe_mm - 1000 * rule["err"]).max(),
                    "pa_err_mm": np.abs(re_mm - 1000 * rule["pa_err"]).max()}
            for k, v in dist.items():
                out[f"{name}/ref32_dist/{k}"] = np.float64(v)
            print(f"{name:14s} seed {seed} N {pred.shape[1]:4d}  ref32_dist " + "  ".join(f"{k} {v:.3g}" for k, v in dist.items()))
        (exempt_names if exempt else names).append(name)
    out["cases"] = np.array(names)
    out["exempt_cases"] = np.array(exempt_names)

    # ---- one Evaluator pass: 21 joints, a 10-joint subset, pelvis 9, two batches
    for seed in range(7000, 8000):
        rng = np.random.default_rng(seed)
        p3, g3 = hand_sets(rng, 21)
        rp, rg = p3 - p3[:, [PELVIS]], g3 - g3[:, [PELVIS]]
        if well_conditioned(rp[:, KEYPOINT_LIST], rg[:, KEYPOINT_LIST]):
            break
    g4 = np.concatenate([g3, np.ones((B, 21, 1), np.float32)], -1)
    g2 = np.concatenate([rng.uniform(-0.5, 0.5, (B, 21, 2)), rng.uniform(0, 1, (B, 21, 1))], -1).astype(np.float32)
    p2 = (g2[:, :, :2] + rng.normal(size=(B, 21, 2)) * 0.02).astype(np.float32)
    metrics = ['mode_mpjpe', 'mode_re', 'min_mpjpe', 'min_re', 'mode_kpl2']
    ev = ref.Evaluator(B, KEYPOINT_LIST, PELVIS, metrics=metrics)
    returned = []
    for lo, hi in ((0, 4), (4, 7)):
        r = ev({'pred_keypoints_3d': torch.from_numpy(p3[lo:hi].copy()), 'pred_keypoints_2d': torch.from_numpy(p2[lo:hi].copy())},
               {'keypoints_3d': torch.from_numpy(g4[lo:hi].copy()), 'keypoints_2d': torch.from_numpy(g2[lo:hi].copy())})
        returned.append(r)
    rule = PR.pose_eval(p3, g4, root=PELVIS, sel=KEYPOINT_LIST)
    kpl2 = (g2[:, :, 2].astype(np.float64) * ((p2.astype(np.float64) - g2[:, :, :2]) ** 2).sum(-1)).mean(-1)
    out.update({"evaluator/pred_keypoints_3d": p3, "evaluator/pred_keypoints_2d": p2, "evaluator/keypoints_3d": g4,
                "evaluator/keypoints_2d": g2, "evaluator/seed": np.int64(seed), "evaluator/metrics": np.array(metrics),
                "evaluator/counter": np.int64(ev.counter)})
    for m in metrics:
        out[f"evaluator/{m}"] = np.asarray(getattr(ev, m), np.float64)
        out[f"evaluator/dict/{m}"] = np.float64(ev.get_metrics_dict()[m])
    out["evaluator/returned_mode_mpjpe"] = np.concatenate([r['mode_mpjpe'] for r in returned])
    out["evaluator/returned_mode_re"] = np.concatenate([r['mode_re'] for r in returned])
    dist = {"mpjpe_mm": np.abs(ev.mode_mpjpe - 1000 * rule["err"]).max(), "re_mm": np.abs(ev.mode_re - 1000 * rule["pa_err"]).max(),
            "kpl2": np.abs(ev.mode_kpl2 - kpl2).max()}
    for k, v in dist.items():
        out[f"evaluator/ref32_dist/{k}"] = np.float64(v)
    print(f"evaluator      seed {seed}  ref32_dist " + "  ".join(f"{k} {v:.3g}" for k, v in dist.items()))
    # the public call signatures (lists of parameter names), so that the tests do not retype them
    import inspect
    for name in ("compute_similarity_transform", "reconstruction_error", "eval_pose", "Evaluator.__init__", "Evaluator.__call__",
                 "EvaluatorPCK.__init__", "EvaluatorPCK.__call__"):
        obj = ref
        for part in name.split("."):
            obj = getattr(obj, part)
        out[f"signatures/{name}"] = np.array(list(inspect.signature(obj).parameters))
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
