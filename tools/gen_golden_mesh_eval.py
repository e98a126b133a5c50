#!/usr/bin/env python3
"""Generate tests/golden/mesh_eval.npz from the REFERENCE's rootnet/KeypointFusion/util/eval_utils.py (loaded by file path
from the reference tree; pure numpy, CPU): get_measures, calc_auc and eval_auc on seeded joint errors.

Cases: N in {1, 37, 1000} samples of 21 keypoints, each with three parameter sets -- (0.0, 0.050, 20) (the defaults),
(0.0, 0.05, 100) (the field's) and (0.0, 0.0625, 17), whose thresholds are the multiples of 1/256.  For the first two the errors
are gamma distributed with a mean of about 16 mm, stored as fp32 on a grid of 2^-16 m; for the third every error is a multiple
of 1/256, so every error lies exactly on a threshold (the <= of _get_pck decides every one of them).  The reference is fed
Python floats that are fp32-representable (its own list-of-lists layout), so that what it compares does not depend on numpy's
scalar promotion rules.  Per case: the inputs, auc_all, pck_curve_all, thresholds and calc_auc(thr[8:] * 1000, curve[8:]).
Then the lines eval_auc prints for a seeded two-stage joint_error_list, and the parameter names of the three public
functions.  Data only, no code."""
import contextlib
import importlib.util
import inspect
import io
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.gen_golden_rootnet import REF  # noqa: E402
OUT = os.path.join(ROOT, "tests", "golden", "mesh_eval.npz")
K = 21
SIZES = (1, 37, 1000)
PARAMS = ((0.0, 0.050, 20), (0.0, 0.05, 100), (0.0, 0.0625, 17))


def load_reference():
    spec = importlib.util.spec_from_file_location("ref_eval_utils", os.path.join(REF, "rootnet", "KeypointFusion", "util", "eval_utils.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def gamma_errors(rng, n):
    """(n, 21) fp32 errors in metres, mean about 16 mm, on a grid of 2^-16 m."""
    return (np.round(rng.gamma(2.0, 0.008, size=(n, K)) * 2.0 ** 16) / 2.0 ** 16).astype(np.float32)


def grid_errors(rng, n):
    """(n, 21) fp32 errors, each a multiple of 1/256 in 0 .. 20/256 (the thresholds end at 16/256)."""
    return (rng.integers(0, 21, size=(n, K)) / 256.0).astype(np.float32)


def as_reference_data(err):
    return [[float(e) for e in err[:, k]] for k in range(err.shape[1])]


def main():
    ref = load_reference()
    out, names = {}, []
    for n in SIZES:
        rng = np.random.default_rng(500 + n)
        inputs = {"gamma": gamma_errors(rng, n), "grid": grid_errors(rng, n)}
        for pi, (val_min, val_max, steps) in enumerate(PARAMS):
            kind = "grid" if pi == 2 else "gamma"
            err = inputs[kind]
            assert np.array_equal(err.astype(np.float64).astype(np.float32), err)
            auc_all, curve, thr = ref.get_measures(as_reference_data(err), val_min, val_max, steps)
            name = f"n{n}_p{pi}"
            out.update({f"{name}/err": f"{kind}{n}", f"{name}/params": np.array([val_min, val_max, steps], np.float64),
                        f"{name}/auc_all": np.float64(auc_all), f"{name}/pck_curve_all": np.asarray(curve, np.float64),
                        f"{name}/thresholds": np.asarray(thr, np.float64),
                        f"{name}/calc_auc_tail": np.float64(ref.calc_auc(thr[8:] * 1000.0, curve[8:]))})
            out[f"inputs/{kind}{n}"] = err
            if kind == "grid":
                assert np.isin(err.astype(np.float64), thr).sum() > 0.7 * err.size          # most errors sit on a threshold
            names.append(name)
            print(f"{name:10s} {kind:5s} N {n:4d} steps {steps:3d}  auc_all {auc_all:.6f}")
    out["cases"] = np.array(names)

    # ---- eval_auc: three items of two stages, errors in mm (its thresholds are 0..50), float64 arrays of fp32 values
    rng = np.random.default_rng(900)
    jel = []
    for i, n in enumerate((5, 4, 7)):
        first = rng.gamma(2.0, 11.0, size=(n, K)).astype(np.float32).astype(np.float64)
        last = rng.gamma(2.0, 7.0, size=(n, K)).astype(np.float32).astype(np.float64)
        jel.append([first, last])
        out[f"eval_auc/first_{i}"], out[f"eval_auc/last_{i}"] = first.astype(np.float32), last.astype(np.float32)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        ref.eval_auc(jel, 16)
    lines = buf.getvalue().splitlines()
    assert len(lines) == 6 and lines[0] == "stage: 0" and lines[3] == "stage: -1"
    out["eval_auc/items"] = np.int64(len(jel))
    out["eval_auc/lines"] = np.array(lines)
    print("\n".join(lines))
    for name in ("eval_auc", "get_measures", "calc_auc"):
        out[f"signatures/{name}"] = np.array(list(inspect.signature(getattr(ref, name)).parameters))
    np.savez_compressed(OUT, **out)
    size = os.path.getsize(OUT)
    assert size < 100_000, size
    print(f"wrote {OUT} ({size} bytes)")


if __name__ == "__main__":
    main()
