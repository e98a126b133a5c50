"""Host checks of the mesh scores (hm_mesh_score, hm_pck_auc, hamer.utils.mesh_eval, evaluate --mesh-scores): the fp64 rule of
tests/mesh_eval_rule.py against the reference's recorded get_measures / calc_auc outputs (tests/golden/mesh_eval.npz, written
by tools/gen_golden_mesh_eval.py) and against hand-made cases, and the surface -- exports, header, build list, argument
checks, signatures, the command-line flag.  No GPU."""
import ctypes as C
import inspect
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_eval_rule as MR  # noqa: E402

from hamer_yolo_amd import build as B  # noqa: E402
from hamer_yolo_amd import lib as L  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", "mesh_eval.npz"))
CASES = [str(c) for c in G["cases"]]


def case_inputs(case):
    val_min, val_max, steps = G[f"{case}/params"]
    return G[f"inputs/{str(G[f'{case}/err'])}"], float(val_min), float(val_max), int(steps)


# ------------------------------------------------------------------ the rule against the reference's outputs
@pytest.mark.parametrize("case", CASES)
def test_rule_get_measures_matches_the_reference(case):
    err, val_min, val_max, steps = case_inputs(case)
    auc_all, curve, thr, pck, auc = MR.get_measures(err, val_min, val_max, steps)
    assert np.array_equal(thr, G[f"{case}/thresholds"]) and np.array_equal(curve, G[f"{case}/pck_curve_all"])
    assert abs(auc_all - float(G[f"{case}/auc_all"])) <= 1e-12
    assert abs(MR.calc_auc(thr[8:] * 1000.0, curve[8:]) - float(G[f"{case}/calc_auc_tail"])) <= 1e-12
    assert pck.shape == (21, steps) and auc.shape == (21,)
    # the reference's list-of-lists layout gives the same
    listed = MR.get_measures([[float(e) for e in err[:, k]] for k in range(err.shape[1])], val_min, val_max, steps)
    assert listed[0] == auc_all and np.array_equal(listed[1], curve)


def test_sorted_form_of_the_rule_equals_the_direct_one():
    rng = np.random.default_rng(3)
    err = rng.gamma(2.0, 0.008, size=(300, 23)).astype(np.float32)
    err[rng.random(err.shape) < 0.05] = np.nan
    err[:, 5] = np.nan                                                                       # a keypoint that is never hit
    err[::7, 2] = np.float32(0.0625 / 4)                                                     # on a threshold of the third set
    for params in ((0.0, 0.050, 20), (0.0, 0.0625, 17), (0.0, 0.05, 256), (0.01, 0.02, 2)):
        a, b = MR.get_measures(err, *params), MR.get_measures_sorted(err, *params)
        assert a[0] == b[0] and all(np.array_equal(x, y) for x, y in zip(a[1:], b[1:])), params
        assert (a[3][5] == 0).all() and a[4][5] == 0
    for case in CASES:
        err, val_min, val_max, steps = case_inputs(case)
        a, b = MR.get_measures(err, val_min, val_max, steps), MR.get_measures_sorted(err, val_min, val_max, steps)
        assert a[0] == b[0] and all(np.array_equal(x, y) for x, y in zip(a[1:], b[1:])), case


def test_fixture_holds_the_cases_it_should():
    assert CASES == [f"n{n}_p{p}" for n in (1, 37, 1000) for p in range(3)]
    assert [tuple(G[f"n37_p{p}/params"]) for p in range(3)] == [(0.0, 0.050, 20.0), (0.0, 0.05, 100.0), (0.0, 0.0625, 17.0)]
    for n in (1, 37, 1000):
        gamma, grid = G[f"inputs/gamma{n}"], G[f"inputs/grid{n}"]
        assert gamma.shape == grid.shape == (n, 21) and gamma.dtype == grid.dtype == np.float32
        assert np.array_equal(grid * 256, np.round(grid * 256)) and not np.isnan(gamma).any()
        thr = G[f"n{n}_p2/thresholds"]
        assert np.array_equal(thr, np.arange(17) / 256.0)                                    # every error <= 16/256 sits on one
    assert 0.012 < G["inputs/gamma1000"].mean() < 0.020
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "mesh_eval.npz")) < 100_000


def test_rule_hand_made():
    # one keypoint, errors 1, 2, 3, 10 against thresholds 0, 2, 4: pck 0, 1/2 (<= counts the 2), 3/4
    auc_all, curve, thr, pck, auc = MR.get_measures(np.array([[1.0], [2.0], [3.0], [10.0]]), 0.0, 4.0, 3)
    assert thr.tolist() == [0.0, 2.0, 4.0] and pck.tolist() == [[0.0, 0.5, 0.75]] and curve.tolist() == [0.0, 0.5, 0.75]
    assert auc_all == (2 * 0.25 + 2 * 0.625) / 4.0
    nan = MR.get_measures(np.array([[np.nan], [1.0]]), 0.0, 4.0, 3)
    assert nan[3].tolist() == [[0.0, 0.5, 0.5]]                                              # a NaN error is a miss
    # two points against one: both pred points are 3 and 4 away from the gt point, the gt point 3 from its nearest
    pred = np.array([[[3.0, 0.0, 0.0], [0.0, 4.0, 0.0]]])
    gt = np.zeros((1, 1, 3))
    r = MR.mesh_score(pred, gt, thresholds=(3.0, 3.5, 5.0))
    assert r["d_pred"].tolist() == [[3.0, 4.0]] and r["d_gt"].tolist() == [[3.0]] and "point_err" not in r
    assert r["n_pred"].tolist() == [[0, 1, 2]] and r["n_gt"].tolist() == [[0, 1, 1]]         # strict <
    assert r["fscore"].tolist() == [[0.0, 2 * 0.5 * 1.0 / 1.5, 1.0]]
    # root and ranges: the root is subtracted from both sets before the ranges are taken
    rng = np.random.default_rng(1)
    p, g = rng.normal(size=(2, 9, 3)), rng.normal(size=(2, 7, 3))
    a = MR.mesh_score(p, g, root=0, pred_range=(2, 9), gt_range=(1, 6))
    b = MR.mesh_score((p - p[:, :1])[:, 2:9], (g - g[:, :1])[:, 1:6])
    assert all(np.array_equal(a[k], b[k]) for k in a)
    nanp = p.copy()
    nanp[1, 4, 2] = np.nan
    c = MR.mesh_score(nanp, g)
    assert np.isnan(c["d_gt"][1]).all() and np.isnan(c["d_pred"][1, 4]) and np.isfinite(c["d_pred"][1, :4]).all()
    assert (c["fscore"][1] == 0).all() and np.array_equal(c["d_pred"][0], MR.mesh_score(p, g)["d_pred"][0])


# ------------------------------------------------------------------ surface
NAMES = ("hm_mesh_score", "hm_pck_auc_workspace_bytes", "hm_pck_auc")


def test_surface():
    header = open(os.path.join(ROOT, "include", "hamer_hip.h")).read()
    lib = L.load()
    for name in NAMES:
        assert re.search(r"\b%s\(" % name, header) and name in L.EXPORTS and hasattr(lib, name), name
    assert "typedef struct hm_mesh_score_args" in header and "typedef struct hm_pck_auc_args" in header
    assert "mesh_eval.hip" in B.SOURCES and os.path.exists(os.path.join(B.CSRC, "mesh_eval.hip"))
    assert re.search(r"#define HM_VERSION 402\b", header) and L.HM_VERSION == 402 and lib.hm_version() == 402
    src = open(os.path.join(B.CSRC, "mesh_eval.hip")).read()
    assert "#pragma clang fp contract(off)" in src and "getenv" not in src and "hipMalloc" not in src
    assert "hipDeviceSynchronize" not in src and "hipStreamSynchronize" not in src
    # the ctypes structs have the header's layout
    assert C.sizeof(L.MeshScoreArgs) == 24 + 40 + 64 + 48 and L.MeshScoreArgs.thresholds.offset == 64 and L.MeshScoreArgs.d_pred.offset == 128
    assert C.sizeof(L.PckAucArgs) == 8 + 24 + 16 + 8 + 48 + 8 and L.PckAucArgs.K.offset == 48 and L.PckAucArgs.pck.offset == 56
    assert lib.hm_pck_auc_workspace_bytes(21, 100) == 21 * 100 * 8 and lib.hm_pck_auc_workspace_bytes(799, 256) == 799 * 256 * 8
    assert lib.hm_pck_auc_workspace_bytes(0, 20) == 0 and lib.hm_pck_auc_workspace_bytes(21, 1) == 0
    assert lib.hm_pck_auc_workspace_bytes(21, 257) == 0


def _score_args(**kw):
    """A valid record over MADE-UP device addresses that are never dereferenced: every case below must fail in hm_mesh_score's
    host part, before any launch (on a machine with a GPU a regressed check would launch over these wild pointers)."""
    a = L.MeshScoreArgs(pred=0x1000, gt=0x2000, transform=None, B=2, P=30, Q=20, gt_stride=3, root=-1, pred_lo=0, pred_n=30,
                        gt_lo=0, gt_n=20, n_thr=2, d_pred=0x3000, d_gt=None, precision=None, recall=None, fscore=None, point_err=None)
    a.thresholds[0], a.thresholds[1] = 0.005, 0.015
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("kw,word", [
    (dict(pred=None), "null"), (dict(gt=None), "null"), (dict(B=0), "B"), (dict(B=-1), "B"), (dict(P=0), "P"), (dict(P=1025), "P"),
    (dict(Q=0), "Q"), (dict(Q=1025), "Q"), (dict(gt_stride=5), "gt_stride"), (dict(gt_stride=2), "gt_stride"),
    (dict(n_thr=9), "8 thresholds"), (dict(n_thr=-1), "8 thresholds"), (dict(n_thr=0, fscore=0x4000), "thresholds"),
    (dict(point_err=0x4000), "equal"), (dict(point_err=0x4000, pred_lo=5, pred_n=21), "equal"),
    (dict(root=-2), "root"), (dict(root=20), "root"), (dict(root=30), "root"),
    (dict(pred_lo=-1), "pred range"), (dict(pred_n=0), "pred range"), (dict(pred_lo=1), "pred range"), (dict(pred_lo=30, pred_n=1), "pred range"),
    (dict(gt_lo=-1), "gt range"), (dict(gt_n=0), "gt range"), (dict(gt_n=21), "gt range"), (dict(gt_lo=2 ** 31 - 1, gt_n=2), "gt range"),
    (dict(d_pred=None), "output"), (dict(pred=0x1002), "aligned"), (dict(transform=0x5001), "aligned"),
])
def test_mesh_score_argument_checks(kw, word):
    lib = L.load()
    rc = lib.hm_mesh_score(C.byref(_score_args(**kw)), None)
    msg = lib.hm_last_error_string().decode()
    assert rc != 0 and "hm_mesh_score" in msg and word in msg, (rc, msg)


def _auc_args(**kw):
    a = L.PckAucArgs(err=0x1000, N=10, ld=21, chunk_rows=0, val_min=0.0, val_max=0.05, K=21, steps=20, pck=0x2000, auc=0x3000,
                     mean_auc=None, curve=None, thresholds=None, workspace=0x4000, workspace_bytes=21 * 20 * 8)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("kw,word", [
    (dict(err=None), "null"), (dict(pck=None), "null"), (dict(auc=None), "null"), (dict(N=0), "N"), (dict(N=-5), "N"),
    (dict(K=0), "K"), (dict(ld=20), "ld"), (dict(steps=1), "steps"), (dict(steps=257), "steps"), (dict(steps=0), "steps"),
    (dict(val_min=0.05), "val_min"), (dict(val_max=float("nan")), "val_min"), (dict(val_max=float("inf")), "val_min"),
    (dict(chunk_rows=-1), "chunk_rows"), (dict(workspace=None), "workspace"), (dict(workspace_bytes=21 * 20 * 8 - 1), "workspace"),
    (dict(workspace=0x4004), "aligned"),
])
def test_pck_auc_argument_checks(kw, word):
    lib = L.load()
    rc = lib.hm_pck_auc(C.byref(_auc_args(**kw)), None)
    msg = lib.hm_last_error_string().decode()
    assert rc != 0 and "hm_pck_auc" in msg and word in msg, (rc, msg)


def test_null_args_records():
    lib = L.load()
    assert lib.hm_mesh_score(None, None) != 0 and "hm_mesh_score" in lib.hm_last_error_string().decode()
    assert lib.hm_pck_auc(None, None) != 0 and "hm_pck_auc" in lib.hm_last_error_string().decode()


# ------------------------------------------------------------------ the Python layer
def test_signatures_equal_the_recorded_ones():
    from hamer_yolo_amd.hamer.utils import mesh_eval as ME
    ref = {k[len("signatures/"):]: [str(n) for n in G[k]] for k in G.files if k.startswith("signatures/")}
    assert sorted(ref) == ["calc_auc", "eval_auc", "get_measures"] and ref["get_measures"] == ["data", "val_min", "val_max", "steps"]
    for name, want in ref.items():
        assert list(inspect.signature(getattr(ME, name)).parameters) == want, name
    p = inspect.signature(ME.get_measures).parameters
    assert (p["val_min"].default, p["val_max"].default, p["steps"].default) == (0.0, 0.050, 20)
    p = inspect.signature(ME.mesh_score).parameters
    assert list(p)[:7] == ["pred", "gt", "root", "pred_range", "gt_range", "transform", "thresholds"]
    assert p["root"].default == -1 and p["thresholds"].default == (0.005, 0.015) and "want" in p
    assert list(inspect.signature(ME.f_score).parameters) == ["pred", "gt", "th"]
    p = inspect.signature(ME.MeshEvaluator.__init__).parameters
    assert list(p) == ["self", "dataset_length", "n_joints", "root", "thresholds", "auc"]
    assert (p["n_joints"].default, p["root"].default, p["thresholds"].default, p["auc"].default) == (21, 0, (0.005, 0.015), (0.0, 0.05, 100))
    c = inspect.signature(ME.MeshEvaluator.__call__).parameters
    assert list(c) == ["self", "pred_points", "gt_points", "sync"] and c["sync"].default is False


def test_evaluator_constructor_and_calc_auc_need_no_gpu():
    from hamer_yolo_amd.hamer.utils import mesh_eval as ME
    ev = ME.MeshEvaluator(10)
    assert ev.counter == 0 and ev.f_names == ["f5", "f15", "pa_f5", "pa_f15"] and ev.auc == (0.0, 0.05, 100)
    assert ME.MeshEvaluator(3, thresholds=(0.0025, 0.01)).f_names == ["f2.5", "f10", "pa_f2.5", "pa_f10"]
    assert all(v.shape == (0,) for v in ev.per_hand().values())
    with pytest.raises(ValueError):
        ev.result()
    for bad in (dict(thresholds=()), dict(thresholds=(0.001,) * 9), dict(auc=(0.0, 0.05, 1)), dict(auc=(0.0, 0.05, 257)),
                dict(auc=(0.05, 0.05, 20)), dict(n_joints=0)):
        with pytest.raises(ValueError):
            ME.MeshEvaluator(4, **bad)
    for case in CASES:
        thr, curve = G[f"{case}/thresholds"], G[f"{case}/pck_curve_all"]
        assert abs(ME.calc_auc(thr[8:] * 1000.0, curve[8:]) - float(G[f"{case}/calc_auc_tail"])) <= 1e-12


def test_evaluate_flag_and_defaults():
    from hamer_yolo_amd import evaluate
    a = evaluate._parser().parse_args(["--pred", "A", "--ref", "B"])
    assert a.mesh_scores is False
    a = evaluate._parser().parse_args(["--pred", "A", "--ref", "B", "--mesh-scores", "--json", "o.json"])
    assert a.mesh_scores is True and a.json == "o.json"
    assert evaluate.METRICS == ("mpjpe", "pa_mpjpe", "mpvpe", "pa_mpvpe", "root", "max_dtheta", "max_dbeta")
    p = inspect.signature(evaluate.compare_folders_with).parameters
    assert list(p) == ["pred_dir", "ref_dir", "hamer", "json_path", "mesh_scores"] and p["mesh_scores"].default is False
    line = evaluate.format_mesh_line({"mesh_scores": {
        "metrics": {k: {"mean": 0.5} for k in ("f5", "f15", "pa_f5", "pa_f15")},
        "auc": {"auc_j": 0.9, "auc_v": 0.8, "pa_auc_j": 0.95, "pa_auc_v": 0.85, "val_min": 0.0, "val_max": 0.05, "steps": 100}}})
    assert all(w in line for w in ("F@5 0.5000", "F@15", "PA-F@5", "PA-F@15", "AUC 0-50 mm", "PA-V 0.8500"))
