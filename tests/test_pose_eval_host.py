"""Host checks of the hand-metric evaluation (hm_pose_eval, hamer.utils.pose_utils, hamer_yolo_amd.evaluate): the fp64 rule of
tests/pose_eval_rule.py against the reference's recorded fp32 outputs (tests/golden/pose_eval.npz, written by
tools/gen_golden_pose_eval.py) and against known answers, the PCK rule on hand-made cases, and the surface -- export, header,
build list, argument checks, lazy package import, signatures, command-line flags, the pairing of two record folders.  No GPU."""
import ctypes as C
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pose_eval_rule as PR  # noqa: E402

from hamer_yolo_amd import build as B  # noqa: E402
from hamer_yolo_amd import lib as L  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", "pose_eval.npz"))
CASES = [str(c) for c in G["cases"]]


# ------------------------------------------------------------------ the rule against the reference's fp32 outputs
@pytest.mark.parametrize("case", CASES)
def test_rule_matches_the_reference(case):
    """Within 2 x ref32_dist (the recorded distance itself, with room for another BLAS / LAPACK build under numpy)."""
    pred, gt = G[f"{case}/pred"], G[f"{case}/gt"]
    r = PR.pose_eval(pred, gt)
    d = lambda k: 2.0 * float(G[f"{case}/ref32_dist/{k}"])                                   # noqa: E731
    assert np.abs(r["aligned"] - G[f"{case}/ref_s1hat"]).max() <= d("s1hat")
    assert np.abs(r["pa_err"] - G[f"{case}/ref_re"]).max() <= d("pa_err")
    assert np.abs(1000 * r["err"] - G[f"{case}/ref_mpjpe_mm"]).max() <= d("err_mm")
    assert np.abs(1000 * r["pa_err"] - G[f"{case}/ref_re_mm"]).max() <= d("pa_err_mm")
    assert float(G[f"{case}/ref32_dist/s1hat"]) < 1e-6 and float(G[f"{case}/ref32_dist/pa_err"]) < 1e-6   # fp32 noise, no more


def test_fixture_cases_meet_the_conditioning_rule():
    for case in CASES:
        _, _, _, _, sign, s = PR.similarity_transform(G[f"{case}/pred"], G[f"{case}/gt"])
        margin = np.where(sign > 0, (s[:, 1] + s[:, 2]) / s[:, 0], (s[:, 1] - s[:, 2]) / s[:, 0])
        assert (margin >= float(G["cond"])).all(), case
    assert {"rand3", "rand21", "rand64", "rand65", "rand778", "rand1024", "similarity", "mirror", "identical"} <= set(CASES)
    assert sorted(str(c) for c in G["exempt_cases"]) == ["planar_mirror", "two"]
    assert all(G[f"{c}/pred"].dtype == np.float32 and len(G[f"{c}/pred"]) == 7 for c in CASES)


def test_rule_matches_the_reference_evaluator():
    kl, pelvis = [int(i) for i in G["keypoint_list"]], int(G["pelvis_ind"])
    assert len(kl) == 10 and pelvis == 9
    r = PR.pose_eval(G["evaluator/pred_keypoints_3d"], G["evaluator/keypoints_3d"], root=pelvis, sel=kl)
    assert np.abs(1000 * r["err"] - G["evaluator/mode_mpjpe"]).max() <= 2 * float(G["evaluator/ref32_dist/mpjpe_mm"])
    assert np.abs(1000 * r["pa_err"] - G["evaluator/mode_re"]).max() <= 2 * float(G["evaluator/ref32_dist/re_mm"])
    assert np.array_equal(G["evaluator/mode_mpjpe"], G["evaluator/min_mpjpe"])              # num_samples is 1 in the reference too
    assert np.array_equal(G["evaluator/mode_re"], G["evaluator/min_re"]) and int(G["evaluator/counter"]) == 7


# ------------------------------------------------------------------ known answers of the rule
def test_rule_known_answers():
    # an exact similarity (fp32 inputs: the residual is the rounding of gt, at most sqrt(3) * 2^-24 * max|gt| per point)
    r = PR.pose_eval(G["similarity/pred"], G["similarity/gt"])
    assert r["pa_err"].max() <= np.sqrt(3.0) * 2.0 ** -24 * np.abs(G["similarity/gt"]).max()
    assert np.abs(r["transform"][:, 0] - 2.5).max() < 1e-5
    # a planar set against its in-plane mirror: a half turn about an in-plane axis fits exactly
    r = PR.pose_eval(G["planar_mirror/pred"], G["planar_mirror/gt"])
    assert r["pa_err"].max() < 1e-12 and r["err"].min() > 1e-3
    assert np.allclose(np.linalg.det(r["transform"][:, 1:10].reshape(-1, 3, 3)), 1.0, atol=1e-12)
    # two points: always an exact fit
    r = PR.pose_eval(G["two/pred"], G["two/gt"])
    assert r["pa_err"].max() < 1e-12 and r["err"].min() > 1e-3
    # identical sets
    r = PR.pose_eval(G["identical/pred"], G["identical/gt"])
    assert r["pa_err"].max() < 1e-12 and (r["err"] == 0).all()
    # the mirror image of a non-planar set: no rotation fits, and R stays proper
    r = PR.pose_eval(G["mirror/pred"], G["mirror/gt"])
    assert r["pa_err"].min() > 1e-3
    assert np.allclose(np.linalg.det(r["transform"][:, 1:10].reshape(-1, 3, 3)), 1.0, atol=1e-12)


def test_rule_degenerate_inputs_give_nan_only_where_the_reference_does():
    rng = np.random.default_rng(0)
    gt = rng.normal(size=(2, 5, 3)).astype(np.float32)
    one = PR.pose_eval(gt[:, :1] + 0.25, gt[:, :1])                                          # N = 1
    same = PR.pose_eval(np.full((2, 5, 3), 0.5, np.float32), gt)                             # coincident predictions
    for r in (one, same):
        assert np.isfinite(r["err"]).all() and (r["err"] > 0).all()
        assert np.isnan(r["pa_err"]).all() and np.isnan(r["aligned"]).all() and np.isnan(r["transform"]).all()


def test_rule_root_and_selection():
    pred, gt = G["rand21/pred"].astype(np.float64), G["rand21/gt"].astype(np.float64)      # widened: the subtraction is fp64
    sel = [1, 4, 7, 20]
    a = PR.pose_eval(pred, gt, root=3, sel=sel)
    b = PR.pose_eval((pred - pred[:, [3]])[:, sel], (gt - gt[:, [3]])[:, sel])
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    assert np.abs(PR.apply_transform(pred, a["transform"], root=3, sel=sel) - a["aligned"]).max() < 1e-15
    assert PR.sel_words(sel, 21)[0] == (1 << 1 | 1 << 4 | 1 << 7 | 1 << 20) and PR.sel_words([64, 1023], 1024)[1] == 1


def test_pck_rule_hand_made():
    gt = np.zeros((4, 3, 2))
    pred = gt.copy()
    pred[:, 0, 0] = [0.01, 0.02, 0.2, 0.3]               # keypoint 0: two of four inside 0.05
    pred[:, 1, 1] = 0.04                                 # keypoint 1: all inside
    mask = np.ones((4, 3), bool)
    mask[:, 2] = False                                   # keypoint 2: no valid sample
    acc, avg, cnt = PR.pck(pred, gt, mask, 0.05)
    assert acc.tolist() == [0.5, 1.0, -1.0] and avg == 0.75 and cnt == 2
    mask[2:, 0] = False                                  # only the two near samples of keypoint 0 stay valid
    acc, avg, cnt = PR.pck(pred, gt, mask, 0.05)
    assert acc.tolist() == [1.0, 1.0, -1.0] and avg == 1.0 and cnt == 2
    acc, avg, cnt = PR.pck(pred, gt, np.zeros((4, 3), bool), 0.05)
    assert acc.tolist() == [-1.0, -1.0, -1.0] and avg == 0.0 and cnt == 0
    acc, _, _ = PR.pck(pred, gt, np.ones((4, 3), bool), 0.04)                                # d < thr is strict
    assert acc[1] == 0.0


# ------------------------------------------------------------------ surface
def test_surface():
    header = open(os.path.join(ROOT, "include", "hamer_hip.h")).read()
    lib = L.load()
    assert re.search(r"\bint hm_pose_eval\(", header) and "typedef struct hm_pose_eval_args" in header
    assert "hm_pose_eval" in L.EXPORTS and hasattr(lib, "hm_pose_eval")
    assert "pose_eval.hip" in B.SOURCES and os.path.exists(os.path.join(B.CSRC, "pose_eval.hip"))
    assert re.search(r"#define HM_VERSION 402\b", header) and L.HM_VERSION == 402 and lib.hm_version() == 402
    # the ctypes struct has the header's layout: 2 pointers, 4 ints, 16 words, 4 pointers
    assert C.sizeof(L.PoseEvalArgs) == 16 + 16 + 128 + 32 and L.PoseEvalArgs.sel.offset == 32 and L.PoseEvalArgs.err.offset == 160
    assert "getenv" not in open(os.path.join(B.CSRC, "pose_eval.hip")).read()


def _args(**kw):
    """A valid argument record over MADE-UP device addresses that are never dereferenced: every check below fails on the host,
    before any launch.  Whoever edits the checks: if one of them regressed and this file ran on a machine with a GPU, the
    kernel would be launched over these wild pointers -- keep every case here failing in hm_pose_eval's host part."""
    a = L.PoseEvalArgs(pred=0x1000, gt=0x2000, B=2, P=21, gt_stride=3, root=-1, err=0x3000, pa_err=None, aligned=None, transform=None)
    for k, v in kw.items():
        if k == "sel":
            for i in v:
                a.sel[i >> 6] |= 1 << (i & 63)
        else:
            setattr(a, k, v)
    return a


@pytest.mark.parametrize("kw,word", [
    (dict(pred=None), "null"), (dict(gt=None), "null"), (dict(B=0), "B"), (dict(B=-3), "B"), (dict(P=0), "P"), (dict(P=1025), "P"),
    (dict(gt_stride=2), "gt_stride"), (dict(gt_stride=5), "gt_stride"), (dict(root=-2), "root"), (dict(root=21), "root"),
    (dict(sel=[21]), "sel"), (dict(sel=[3, 64]), "sel"), (dict(sel=[1023]), "sel"), (dict(P=1024, sel=[1023], root=1024), "root"),
    (dict(err=None), "output"), (dict(pred=0x1002), "aligned"), (dict(gt=0x2001), "aligned"),
])
def test_argument_checks(kw, word):
    lib = L.load()
    rc = lib.hm_pose_eval(C.byref(_args(**kw)), None)
    msg = lib.hm_last_error_string().decode()
    assert rc != 0 and "hm_pose_eval" in msg and word in msg, (rc, msg)


def test_null_args_record():
    lib = L.load()
    assert lib.hm_pose_eval(None, None) != 0 and "hm_pose_eval" in lib.hm_last_error_string().decode()


def test_package_import_is_lazy_and_the_names_resolve():
    code = ("import sys; import hamer_yolo_amd.hamer.utils as U; "
            "assert 'hamer_yolo_amd.lib' not in sys.modules and 'hamer_yolo_amd.hamer.utils.pose_utils' not in sys.modules; "
            "assert 'torch' not in sys.modules; "
            "from hamer_yolo_amd.hamer.utils import Evaluator, eval_pose; from hamer_yolo_amd import lib; assert lib._lib is None; "
            "import hamer_yolo_amd.compat as compat; compat.install(); "
            "from hamer.utils.pose_utils import Evaluator as E2, EvaluatorPCK, compute_similarity_transform, reconstruction_error; "
            "from hamer.utils import eval_pose as e2, Evaluator as E3; "
            "assert E2 is Evaluator and E3 is Evaluator and e2 is eval_pose and lib._lib is None; print('ok')")
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr
    import hamer_yolo_amd.hamer.utils as U
    with pytest.raises(AttributeError):
        U.no_such_name


# the reference's signatures (hamer/utils/pose_utils.py:9, :60, :73, :91-96, :146, :228, :287) as the fixture generator
# read them off the reference's module; Evaluator.__call__ gains `sync`
REF_SIGNATURES = {k[len("signatures/"):]: [str(n) for n in G[k]] for k in G.files if k.startswith("signatures/")}
REF_SIGNATURES["Evaluator.__call__"] = REF_SIGNATURES["Evaluator.__call__"] + ["sync"]


def test_signatures_equal_the_reference():
    from hamer_yolo_amd.hamer.utils import pose_utils as PU
    assert len(REF_SIGNATURES) == 7 and REF_SIGNATURES["eval_pose"] == ["pred_joints", "gt_joints"]
    for name, want in REF_SIGNATURES.items():
        obj = PU
        for part in name.split("."):
            obj = getattr(obj, part)
        assert list(inspect.signature(obj).parameters) == want, name
    p = inspect.signature(PU.Evaluator.__init__).parameters
    assert p["metrics"].default == ['mode_mpjpe', 'mode_re', 'min_mpjpe', 'min_re'] and p["pck_thresholds"].default is None
    c = inspect.signature(PU.Evaluator.__call__).parameters
    assert c["opt_output"].default is None and c["sync"].default is True
    assert inspect.signature(PU.EvaluatorPCK.__init__).parameters["thresholds"].default == [0.05, 0.1, 0.2, 0.3, 0.4, 0.5]
    for name in ("log", "get_metrics_dict"):
        assert callable(getattr(PU.Evaluator, name)) and callable(getattr(PU.EvaluatorPCK, name))
    assert callable(PU.EvaluatorPCK.compute_pcks)


def test_evaluator_constructor_checks_need_no_gpu():
    from hamer_yolo_amd.hamer.utils.pose_utils import Evaluator
    with pytest.raises(ValueError, match="twice"):
        Evaluator(4, [0, 1, 1], 0)
    with pytest.raises(ValueError):
        Evaluator(4, [0, 1024], 0)
    with pytest.raises(ValueError):
        Evaluator(4, [-1, 2], 0)
    ev = Evaluator(4, [0, 1, 2], 0, metrics=['mode_mpjpe', 'mode_re', 'mode_kpl2'], pck_thresholds=[0.1])
    assert ev.counter == 0 and ev.dataset_length == 4 and ev.pck_evaluator.thresholds == [0.1]
    assert ev.mode_mpjpe.shape == (4,) and ev.mode_mpjpe.dtype == np.float64 and not ev.mode_kpl2.any()
    assert not hasattr(ev, "min_re")
    assert isinstance(type(ev).mode_mpjpe, property) and ev.mode_mpjpe is not ev.mode_mpjpe          # read-only copies
    with pytest.raises(AttributeError):
        ev.mode_mpjpe = np.ones(4)
    assert Evaluator(3, [0], 0, metrics=['mode_mpjpe', 'my_metric']).my_metric.shape == (3,)        # an unknown name: zeros, as the reference


def test_evaluate_parser():
    from hamer_yolo_amd import evaluate
    a = evaluate._parser().parse_args(["--pred", "A", "--ref", "B"])
    assert (a.pred, a.ref, a.json, a.ckpt) == ("A", "B", None, None)
    a = evaluate._parser().parse_args(["--pred", "A", "--ref", "B", "--json", "o.json", "--ckpt", "synthetic:0"])
    assert a.json == "o.json" and a.ckpt == "synthetic:0"
    with pytest.raises(SystemExit):
        evaluate._parser().parse_args(["--pred", "A"])
    assert list(inspect.signature(evaluate.compare_folders).parameters) == ["pred_dir", "ref_dir", "hamer", "json_path"]


def _hand(seed, right):
    rng = np.random.default_rng(seed)
    pg, ph = rng.normal(size=3) * 0.1, rng.normal(size=45) * 0.1
    return {'betas': rng.normal(size=10), 'theta': np.concatenate((pg, ph)), 'pose_hand': ph, 'pose_global': pg,
            'cam_t': rng.normal(size=3), 'is_right': right}


def test_evaluate_pairing(tmp_path):
    from hamer_yolo_amd import evaluate
    a, b = tmp_path / "a", tmp_path / "b"
    a.mkdir(), b.mkdir()
    np.save(a / "f0.npy", {'left': _hand(1, False), 'right': _hand(2, True)})
    np.save(b / "f0.npy", {'left': _hand(3, False), 'right': _hand(4, True)})               # both sides present
    np.save(a / "f1.npy", {'left': None, 'right': _hand(5, True)})
    np.save(b / "f1.npy", {'left': _hand(6, False), 'right': _hand(7, True)})               # a hand on one side only
    np.save(a / "f2.npy", {'left': _hand(8, False), 'right': None})                         # a file the other folder lacks
    np.save(b / "f3.npy", {'left': None, 'right': None})                                    # a file without hands
    pairs, only_pred, only_ref = evaluate.pair_records(str(a), str(b))
    assert [(p[0], p[1]) for p in pairs] == [("f0", "left"), ("f0", "right"), ("f1", "right")]
    assert only_pred == [("f2", "left")] and only_ref == [("f1", "left")]
    assert pairs[0][2]['is_right'] is False and np.array_equal(pairs[2][3]['betas'], _hand(7, True)['betas'])
    s = evaluate.summary([1.0, 2.0, 3.0, 10.0])
    assert s["mean"] == 4.0 and s["median"] == 2.5 and s["max"] == 10.0 and s["p95"] == pytest.approx(8.95)
    assert all(np.isnan(v) for v in evaluate.summary([]).values())
