"""GPU: hm_mesh_score and hm_pck_auc against the fp64 rules of tests/mesh_eval_rule.py at the sizes where the indexing can go
wrong, their edge cases and their batch / chunk invariance; the Python layer (hamer.utils.mesh_eval) against the reference's
recorded outputs (tests/golden/mesh_eval.npz); evaluate --mesh-scores end to end on synthetic weights.

Bounds.  The kernels evaluate in fp64 in the rule's order and round to fp32 once at the store, so a distance is within half an
fp32 ulp of the rule's (``one_rounding`` of tests/test_gpu_pose_eval.py: 2^-24 |want| (1 + 2^-10) + 1e-12).  Threshold counts
are integers and must be equal, on the condition -- asserted by each test on its own inputs with the rule -- that no rule
distance lies within 1e-9 (relative) of a threshold.  PCK values are count / N with one division and must be equal; an AUC is at
most 256 terms of size <= 1 summed in another order than numpy's, 1.1e-16 each: 1e-12."""
import os
import shutil

import numpy as np
import pytest
import torch

import mesh_eval_rule as MR
import pose_eval_rule as PR
from hamer_yolo_amd import lib as L
from hamer_yolo_amd.hamer.utils import mesh_eval as ME
from hamer_yolo_amd.hamer.utils import pose_utils as PU

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", "mesh_eval.npz"))
CASES = [str(c) for c in G["cases"]]
H = 2.0 ** -24
THR = (0.005, 0.015)
EVERY = ("d_pred", "d_gt", "precision", "recall", "fscore")


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32).to(DEV)


def run(pred, gt, want=EVERY, transform=None, **kw):
    o = ME.mesh_score(dev(pred), dev(gt), want=want, transform=None if transform is None else dev(transform), **kw)
    return {k: v.cpu().numpy() for k, v in o.items()}


def one_rounding(got, want, what=""):
    """got (fp32) is the fp64 value `want` rounded once."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    bad = np.abs(got - want) > H * np.abs(want) * (1 + 2.0 ** -10) + 1e-12
    assert not (bad & ~np.isnan(want)).any(), (what, float(np.nanmax(np.abs(got - want))))


def same_bytes(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def clouds(seed, B, P, Q):
    """Hand-sized clouds (metres) around a common point half a metre away; with P == Q the prediction is the ground truth plus
    8 mm of noise and a shift (tests/test_gpu_pose_eval.hands), otherwise two clouds drawn apart."""
    rng = np.random.default_rng(seed)
    centre = rng.normal(size=(B, 1, 3)) * 0.1 + np.array([0.0, 0.0, 0.5])
    gt = rng.normal(size=(B, Q, 3)) * 0.04 + centre
    if P == Q:
        pred = gt + rng.normal(size=(B, P, 3)) * 0.008 + rng.normal(size=(B, 1, 3)) * 0.004
    else:
        pred = rng.normal(size=(B, P, 3)) * 0.04 + centre + rng.normal(size=(B, 1, 3)) * 0.004
    return pred.astype(np.float32), gt.astype(np.float32)


def against_the_rule(got, rule, n_p, n_g, thresholds=THR, what=""):
    assert MR.threshold_margin(rule, thresholds) > 1e-9, what                 # the test's own condition on its inputs
    for k in ("d_pred", "d_gt", "point_err"):
        if k in got:
            one_rounding(got[k], rule[k], f"{what} {k}")
    assert np.array_equal(np.rint(got["precision"].astype(np.float64) * n_p), rule["n_pred"]), what
    assert np.array_equal(np.rint(got["recall"].astype(np.float64) * n_g), rule["n_gt"]), what
    for k in ("precision", "recall", "fscore"):
        one_rounding(got[k], rule[k], f"{what} {k}")


# ------------------------------------------------------------------ hm_mesh_score: sizes
@pytest.mark.parametrize("P,Q", [(1, 1), (1, 3), (3, 1), (64, 64), (65, 64), (255, 257), (778, 778), (1024, 1024), (1024, 1)])
def test_sizes(P, Q):
    pred, gt = clouds(100 + P + 2 * Q, 5, P, Q)
    want = EVERY + (("point_err",) if P == Q else ())
    got, rule = run(pred, gt, want=want, thresholds=THR), MR.mesh_score(pred, gt, thresholds=THR)
    assert got["d_pred"].shape == (5, P) and got["d_gt"].shape == (5, Q) and got["fscore"].shape == (5, 2)
    against_the_rule(got, rule, P, Q, what=f"{P}x{Q}")
    if min(P, Q) >= 64:
        assert 0 < got["fscore"][:, 1].min() and got["fscore"][:, 0].max() < 1      # the thresholds cut through the data
    if P != Q:
        with pytest.raises(L.HipLibraryError, match="equal"):
            run(pred, gt, want=("point_err",))


def test_deliberate_tie():
    gt, pred, t = np.zeros((1, 1, 3), np.float32), np.array([[[2.0 ** -7, 0.0, 0.0]]], np.float32), 2.0 ** -7
    got = run(pred, gt, want=EVERY + ("point_err",), thresholds=(t, t * (1 + 2.0 ** -52)))
    assert got["d_pred"][0, 0] == t and got["d_gt"][0, 0] == t and got["point_err"][0, 0] == t
    assert got["fscore"].tolist() == [[0.0, 1.0]] and got["precision"].tolist() == [[0.0, 1.0]]      # strict <
    o = ME.pck_auc(dev(np.array([[t]])), 0.0, 2.0 ** -6, 3)                                          # thresholds 0, 2^-7, 2^-6
    assert o["thresholds"].cpu().tolist() == [0.0, t, 2 * t] and o["pck"].cpu().tolist() == [[0.0, 1.0, 1.0]]      # <=
    assert o["auc"].cpu().tolist() == [0.75] and o["mean_auc"].item() == 0.75


def test_batch_invariance():
    pred, gt = clouds(7, 64, 778, 778)
    tr = np.random.default_rng(8).normal(size=(64, 13)).astype(np.float32)
    want = EVERY + ("point_err",)
    for transform in (None, tr):
        alone = run(pred[3:4], gt[3:4], want=want, transform=None if transform is None else transform[3:4])
        for B in (1, 2, 5, 7, 64):
            at = 3 if B > 3 else B - 1                                         # hand 3 of 7, and the same hand elsewhere
            p, g = pred[:B].copy(), gt[:B].copy()
            t = None if transform is None else transform[:B].copy()
            p[at], g[at] = pred[3], gt[3]
            if t is not None:
                t[at] = transform[3]
            got = run(p, g, want=want, transform=t)
            for k in want:
                assert same_bytes(got[k][at:at + 1], alone[k]), (B, k)


def test_permuting_the_ground_truth():
    pred, gt = clouds(9, 5, 255, 257)
    perm = np.random.default_rng(10).permutation(257)
    a, b = run(pred, gt), run(pred, gt[:, perm])
    assert same_bytes(a["d_pred"], b["d_pred"]) and same_bytes(a["d_gt"][:, perm], b["d_gt"])
    for k in ("precision", "recall", "fscore"):
        assert same_bytes(a[k], b[k]), k


def test_identical_sets():
    _, gt = clouds(11, 5, 778, 778)
    got = run(gt, gt, want=EVERY + ("point_err",))
    assert all((got[k] == 0).all() for k in ("d_pred", "d_gt", "point_err"))
    assert all((got[k] == 1).all() for k in ("precision", "recall", "fscore"))


def test_similarity_copy():
    rng = np.random.default_rng(12)
    pred, _ = clouds(12, 5, 65, 65)
    c, s = np.cos(0.7), np.sin(0.7)
    R = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]]) @ np.array([[1.0, 0.0, 0.0], [0.0, c, -s], [0.0, s, c]])
    gt = (2.5 * pred.astype(np.float64) @ R.T + np.array([0.3, -0.4, 0.5]) + rng.normal(size=(5, 1, 3)) * 0.01).astype(np.float32)
    raw = run(pred, gt)
    assert (raw["fscore"][:, 0] == 0).all() and raw["d_pred"].min() > 0.1
    tr = PU.pose_eval(dev(pred), dev(gt), want=("transform",))["transform"]
    o = ME.mesh_score(dev(pred), dev(gt), transform=tr, want=EVERY + ("point_err",))
    got, tr = {k: v.cpu().numpy() for k, v in o.items()}, tr.cpu().numpy()
    assert np.abs(tr[:, 0] - 2.5).max() < 1e-5 and (got["fscore"] == 1).all() and got["point_err"].max() < 1e-6
    rule = MR.mesh_score(pred, gt, transform=tr)                               # the stored fp32 transform, widened
    against_the_rule(got, rule, 65, 65, what="similarity")


def test_root_and_ranges_of_the_driver():
    pred, gt = clouds(13, 5, 799, 799)
    verts, joints = (21, 799), (0, 21)
    got = run(pred, gt, want=EVERY + ("point_err",), root=0, pred_range=verts, gt_range=verts)
    assert got["d_pred"].shape == (5, 778) and got["point_err"].shape == (5, 778)
    against_the_rule(got, MR.mesh_score(pred, gt, root=0, pred_range=verts, gt_range=verts), 778, 778, what="vertices")
    tr = PU.pose_eval(dev(pred), dev(gt), root=0, sel=range(*verts), want=("transform",))["transform"].cpu().numpy()
    got = run(pred, gt, want=EVERY + ("point_err",), root=0, pred_range=verts, gt_range=verts, transform=tr)
    against_the_rule(got, MR.mesh_score(pred, gt, root=0, pred_range=verts, gt_range=verts, transform=tr), 778, 778, what="aligned")
    # other roots and lopsided ranges; a range object works as the pair does
    got = run(pred, gt, root=798, pred_range=range(5, 300), gt_range=(700, 799))
    against_the_rule(got, MR.mesh_score(pred, gt, root=798, pred_range=(5, 300), gt_range=(700, 799)), 295, 99, what="lopsided")
    got = run(pred, gt, want=("point_err", "fscore"), root=0, pred_range=joints, gt_range=joints)
    one_rounding(got["point_err"], MR.mesh_score(pred, gt, root=0, pred_range=joints, gt_range=joints)["point_err"], "joints")
    with pytest.raises(ValueError):
        run(pred, gt, pred_range=(21, 800))


def test_gt_stride_4_never_reads_the_fourth_component():
    pred, gt = clouds(14, 5, 65, 64)
    gt4 = np.concatenate([gt, np.full((5, 64, 1), np.nan, np.float32)], -1)
    a, b = run(pred, gt, root=2, gt_range=(1, 64)), run(pred, gt4, root=2, gt_range=(1, 64))
    for k in EVERY:
        assert np.isfinite(b[k]).all() and same_bytes(a[k], b[k]), k


def test_nan_containment():
    pred, gt = clouds(15, 7, 65, 65)
    clean = run(pred, gt, want=EVERY + ("point_err",))
    pred[1, 40, 1] = np.nan
    gt[4, 64, 2] = np.nan
    got = run(pred, gt, want=EVERY + ("point_err",))
    for b in (0, 2, 3, 5, 6):
        for k in got:
            assert np.isfinite(got[k][b]).all() and same_bytes(got[k][b], clean[k][b]), (b, k)
    # hand 1: a NaN pred point is its own distance and every gt point's; hand 4: the other way round
    assert np.isnan(got["d_gt"][1]).all() and np.isnan(got["d_pred"][1, 40]) and np.isfinite(np.delete(got["d_pred"][1], 40)).all()
    assert np.isnan(got["d_pred"][4]).all() and np.isnan(got["d_gt"][4, 64]) and np.isfinite(np.delete(got["d_gt"][4], 64)).all()
    assert np.isnan(got["point_err"][1, 40]) and np.isnan(got["point_err"][4, 64])
    assert (got["fscore"][[1, 4]] == 0).all() and (got["recall"][1] == 0).all() and (got["precision"][4] == 0).all()
    rule = MR.mesh_score(pred, gt, thresholds=THR)
    for k in ("d_pred", "d_gt", "point_err", "precision", "recall", "fscore"):
        one_rounding(got[k], rule[k], k)


def test_f_score_function():
    pred, gt = clouds(16, 5, 255, 257)
    f, p, r = ME.f_score(torch.from_numpy(pred).double(), gt, 0.015)                                  # host inputs are taken
    assert all(t.is_cuda and t.dtype == torch.float32 and tuple(t.shape) == (5,) for t in (f, p, r))
    rule = MR.mesh_score(pred, gt, thresholds=(0.015,))
    for got, k in ((f, "fscore"), (p, "precision"), (r, "recall")):
        one_rounding(got.cpu().numpy(), rule[k][:, 0], k)
    with pytest.raises(L.HipLibraryError):
        ME.mesh_score(torch.from_numpy(pred), torch.from_numpy(gt))                                  # no CPU path


# ------------------------------------------------------------------ hm_pck_auc
def case_inputs(case):
    val_min, val_max, steps = G[f"{case}/params"]
    return G[f"inputs/{str(G[f'{case}/err'])}"], float(val_min), float(val_max), int(steps)


@pytest.mark.parametrize("case", CASES)
def test_get_measures_on_the_fixture(case):
    err, val_min, val_max, steps = case_inputs(case)
    auc_all, curve, thr = ME.get_measures(torch.from_numpy(err), val_min, val_max, steps)
    assert isinstance(auc_all, float) and isinstance(curve, np.ndarray) and isinstance(thr, np.ndarray) and curve.dtype == np.float64
    assert np.array_equal(thr, G[f"{case}/thresholds"]) and np.array_equal(curve, G[f"{case}/pck_curve_all"])
    assert abs(auc_all - float(G[f"{case}/auc_all"])) <= 1e-12
    assert abs(ME.calc_auc(thr[8:] * 1000.0, curve[8:]) - float(G[f"{case}/calc_auc_tail"])) <= 1e-12
    if err.shape[0] <= 37:                                                      # the reference's list of per-keypoint lists
        listed = ME.get_measures([[float(e) for e in err[:, k]] for k in range(21)], val_min, val_max, steps)
        assert listed[0] == auc_all and np.array_equal(listed[1], curve) and np.array_equal(listed[2], thr)
    if steps == 20:
        assert ME.get_measures(err)[0] == auc_all                               # the defaults are the reference's


def errors(seed, N, K):
    rng = np.random.default_rng(seed)
    err = rng.gamma(2.0, 0.008, size=(N, K)).astype(np.float32)
    err[rng.random(err.shape) < 0.02] = np.nan                                 # a NaN error is a miss
    err[rng.random(err.shape) < 0.02] = np.float32(0.0625)                     # on the last threshold exactly
    err[rng.random(err.shape) < 0.02] = 0.0                                    # on the first
    return err


@pytest.mark.parametrize("K", [1, 21, 64, 65, 778, 799])
@pytest.mark.parametrize("N", [1, 255, 257, 4097])
def test_pck_auc_against_the_rule(N, K):
    err = errors(1000 * K + N, N, K)
    d = dev(err)
    for steps in (2, 20, 100, 256):
        o = {k: v.cpu().numpy() for k, v in ME.pck_auc(d, 0.0, 0.0625, steps).items()}
        auc_all, curve, thr, pck, auc = MR.get_measures_sorted(err, 0.0, 0.0625, steps)
        assert o["pck"].shape == (K, steps) and np.array_equal(o["thresholds"], thr), steps
        assert np.array_equal(o["pck"], pck) and np.array_equal(o["curve"], curve), steps
        assert np.abs(o["auc"] - auc).max() <= 1e-12 and abs(o["mean_auc"][0] - auc_all) <= 1e-12, steps


def test_a_nan_error_is_a_miss():
    err = np.array([[0.01, np.nan], [np.nan, np.nan], [0.03, np.nan], [0.2, np.nan]], np.float32)
    o = ME.pck_auc(dev(err), 0.0, 0.04, 3)
    assert o["pck"].cpu().tolist() == [[0.0, 0.25, 0.5], [0.0, 0.0, 0.0]] and o["auc"].cpu().tolist()[1] == 0.0
    assert o["curve"].cpu().tolist() == [0.0, 0.125, 0.25]
    with pytest.raises(ValueError):
        ME.pck_auc(dev(np.zeros((0, 21))))
    with pytest.raises(L.HipLibraryError, match="steps"):
        ME.pck_auc(dev(err), 0.0, 0.04, 257)


def test_chunking_changes_no_byte():
    err = errors(5, 4097, 65)
    wide = dev(np.concatenate([err, np.full((4097, 7), np.nan, np.float32)], 1))      # a leading dimension above K
    base = {k: v.cpu().numpy() for k, v in ME.pck_auc(dev(err), 0.0, 0.05, 100).items()}
    _, _, _, pck, _ = MR.get_measures_sorted(err, 0.0, 0.05, 100)
    assert np.array_equal(base["pck"], pck)
    for chunk, e in ((1, dev(err)), (7, dev(err)), (256, wide[:, :65]), (4096, dev(err)), (4097, wide[:, :65]), (10 ** 9, dev(err))):
        got = {k: v.cpu().numpy() for k, v in ME.pck_auc(e, 0.0, 0.05, 100, chunk_rows=chunk).items()}
        for k in base:
            assert np.array_equal(got[k].view(np.uint64), base[k].view(np.uint64)), (chunk, k)


def test_eval_auc_prints_the_references_lines(capsys):
    jel = [[G[f"eval_auc/first_{i}"], G[f"eval_auc/last_{i}"]] for i in range(int(G["eval_auc/items"]))]
    ME.eval_auc(jel, 16)
    assert capsys.readouterr().out.splitlines() == [str(s) for s in G["eval_auc/lines"]]


# ------------------------------------------------------------------ MeshEvaluator
def test_mesh_evaluator_batches_and_rule():
    pred, gt = clouds(20, 7, 799, 799)
    one, two = ME.MeshEvaluator(7), ME.MeshEvaluator(9)
    r1 = one(torch.from_numpy(pred), torch.from_numpy(gt), sync=True)
    parts = [two(dev(pred[lo:hi]), dev(gt[lo:hi])) for lo, hi in ((0, 4), (4, 7))]
    assert sorted(r1) == ["f15", "f5", "pa_f15", "pa_f5"] and all(isinstance(v, np.ndarray) and v.shape == (7,) for v in r1.values())
    assert all(torch.is_tensor(v) and v.is_cuda and tuple(v.shape) == (n,) for part, n in zip(parts, (4, 3)) for v in part.values())
    assert one.counter == two.counter == 7
    for k in r1:
        assert np.array_equal(np.concatenate([p[k].cpu().numpy() for p in parts]), r1[k]), k
        assert np.array_equal(one.per_hand()[k], r1[k].astype(np.float64)) and np.array_equal(two.per_hand()[k], one.per_hand()[k])
    a, b = one.result(), two.result()
    assert a == b and sorted(a) == sorted(["f5", "f15", "pa_f5", "pa_f15", "auc_j", "auc_v", "pa_auc_j", "pa_auc_v"])
    with pytest.raises(ValueError, match="dataset_length"):
        one(dev(pred[:1]), dev(gt[:1]))
    two(dev(pred[:2]), dev(gt[:2]))
    with pytest.raises(ValueError, match="dataset_length"):
        two(dev(pred[:1]), dev(gt[:1]))
    assert one.counter == 7 and one.result() == a and two.counter == 9
    # against the rule: each set aligned on itself, with the transform hm_pose_eval stored
    verts, joints = (21, 799), (0, 21)
    for name, rng_, key in (("v", verts, "auc_v"), ("j", joints, "auc_j")):
        tr = PU.pose_eval(dev(pred), dev(gt), root=0, sel=range(*rng_), want=("transform",))["transform"].cpu().numpy()
        raw = MR.mesh_score(pred, gt, root=0, pred_range=rng_, gt_range=rng_)
        pa = MR.mesh_score(pred, gt, root=0, pred_range=rng_, gt_range=rng_, transform=tr)
        for rule, prefix in ((raw, ""), (pa, "pa_")):
            if name == "v":
                assert MR.threshold_margin(rule, THR) > 1e-9
                for j, t in enumerate(("f5", "f15")):
                    one_rounding(r1[prefix + t], rule["fscore"][:, j], prefix + t)
                    assert abs(a[prefix + t] - r1[prefix + t].astype(np.float64).mean()) <= 1e-15
            e = rule["point_err"].astype(np.float32)                            # the evaluator keeps the errors as fp32
            assert abs(a[prefix + key] - MR.get_measures_sorted(e, 0.0, 0.05, 100)[0]) <= 1e-12, prefix + key
    assert 0 < a["f5"] < a["pa_f5"] <= 1 and 0 < a["auc_v"] < a["pa_auc_v"] < 1


# ------------------------------------------------------------------ evaluate --mesh-scores, synthetic weights
class _Cfg:
    ckpt_path = "synthetic:0"
    model_cfg = None
    use_onnx = False
    onnx_path = None


class _FixedDetector:
    def __init__(self, dets):
        self.dets = dets

    def detect(self, image):
        return [None], [self.dets]


def test_compare_folders_mesh_scores(tmp_path, monkeypatch, capsys):
    import json
    from PIL import Image
    from hamer_yolo_amd import evaluate, infer, synth
    hi = infer.hamer_inference(_Cfg)
    img_dir, a_dir, b_dir = tmp_path / "rgb", tmp_path / "a", tmp_path / "b"
    img_dir.mkdir()
    for i in range(2):
        Image.fromarray(synth.frame_u8(240, 320, seed=90 + i).numpy()[:, :, ::-1]).save(img_dir / f"f{i}.png")
    dets = [["right", [60.0, 50.0, 120.0, 120.0]], ["left", [190.0, 90.0, 250.0, 160.0]]]
    infer.process_batch_manopara(str(img_dir), str(a_dir), None, hamer=hi, detector=_FixedDetector(dets))
    shutil.copytree(a_dir, b_dir)
    rec0 = np.load(b_dir / "f0.npy", allow_pickle=True).item()
    rec0['right']['betas'] = (rec0['right']['betas'] + 0.5).astype(rec0['right']['betas'].dtype)
    np.save(b_dir / "f0.npy", rec0)

    names = ["f5", "f15", "pa_f5", "pa_f15"]
    plain = evaluate.compare_folders(str(a_dir), str(b_dir), hi)
    assert "mesh_scores" not in plain and "mesh_scores" not in evaluate.compare_folders_with(str(a_dir), str(b_dir), hi)
    out_json = tmp_path / "r.json"
    r = evaluate.compare_folders_with(str(a_dir), str(b_dir), hi, json_path=str(out_json), mesh_scores=True)
    assert json.load(open(out_json)) == r
    assert sorted(r) == sorted(list(plain) + ["mesh_scores"]) and all(r[k] == plain[k] for k in plain)
    ms = r["mesh_scores"]
    assert sorted(ms) == ["auc", "metrics", "per_hand"] and list(ms["per_hand"]) == names and list(ms["metrics"]) == names
    assert sorted(ms["auc"]) == sorted(["auc_j", "auc_v", "pa_auc_j", "pa_auc_v", "val_min", "val_max", "steps"])
    assert (ms["auc"]["val_min"], ms["auc"]["val_max"], ms["auc"]["steps"]) == (0.0, 0.05, 100)
    assert all(sorted(ms["metrics"][k]) == sorted(evaluate.STATS) and len(ms["per_hand"][k]) == 4 for k in names)

    same = evaluate.compare_folders_with(str(a_dir), str(a_dir), hi, mesh_scores=True)["mesh_scores"]
    assert all(same["per_hand"][k] == [1.0] * 4 and all(v == 1.0 for v in same["metrics"][k].values()) for k in names)
    assert all(same["auc"][k] == 1.0 for k in ("auc_j", "auc_v", "pa_auc_j", "pa_auc_v"))

    at = {h: i for i, h in enumerate(r["hands"])}
    for h in ("f0/left", "f1/left", "f1/right"):                                             # untouched hands
        assert all(ms["per_hand"][k][at[h]] == 1.0 for k in names), h
    i = at["f0/right"]
    assert ms["per_hand"]["f5"][i] < 1 and ms["metrics"]["f5"]["mean"] < 1 and all(ms["auc"][k] < 1 for k in ("auc_j", "auc_v"))
    # the perturbed hand against the rule on points rebuilt by mano_hand_joints_vertices (a right hand: no mirroring)
    a0 = np.load(a_dir / "f0.npy", allow_pickle=True).item()
    pts = []
    for hd in (a0['right'], rec0['right']):
        j, v = infer.mano_hand_joints_vertices(hi, [hd])
        pts.append(torch.cat([j, v], 1).float().cpu().numpy())
    assert pts[0].shape == (1, 799, 3)
    verts = (21, 799)
    tr = PU.pose_eval(dev(pts[0]), dev(pts[1]), root=0, sel=range(*verts), want=("transform",))["transform"].cpu().numpy()
    raw = MR.mesh_score(pts[0], pts[1], root=0, pred_range=verts, gt_range=verts)
    pa = MR.mesh_score(pts[0], pts[1], root=0, pred_range=verts, gt_range=verts, transform=tr)
    assert MR.threshold_margin(raw, THR) > 1e-9 and MR.threshold_margin(pa, THR) > 1e-9
    got = np.array([ms["per_hand"][k][i] for k in names])
    one_rounding(got, np.concatenate([raw["fscore"][0], pa["fscore"][0]]), "the perturbed hand")

    # the command line, on the same model
    monkeypatch.setattr(infer, "hamer_inference", lambda cfg: hi)
    capsys.readouterr()                                                                      # what the folder driver printed
    res = evaluate.main(["--pred", str(a_dir), "--ref", str(b_dir)])
    lines = capsys.readouterr().out.splitlines()
    assert "mesh_scores" not in res and len(lines) == 1 and res["per_hand"] == plain["per_hand"]
    res = evaluate.main(["--pred", str(a_dir), "--ref", str(b_dir), "--mesh-scores"])
    lines = capsys.readouterr().out.splitlines()
    assert res["mesh_scores"] == ms and len(lines) == 2 and lines[0] == evaluate.format_line(plain)
    assert all(w in lines[1] for w in ("F@5", "F@15", "PA-F@5", "AUC"))
