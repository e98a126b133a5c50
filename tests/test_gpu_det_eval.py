"""GPU: hm_det_match, hm_det_ap and hm_det_ap_curve against the CPU rule (tests/det_eval_rule.py), the Python layer
(hamer_yolo_amd.yolo.metrics) against the reference's recorded outputs (tests/golden/det_eval.npz), and the detector scored
end to end on synthetic weights.

Bounds.  The match is compared exactly: ``correct`` and ``matched`` equal, ``best_iou`` bit for bit -- every fp32 operation of
the IoU is a single IEEE operation in the rule's order.  AP, p and r are held to 1e-12 absolute.  That bound is derived, not
measured: the inputs of every division are exact integers (or fp32 confidences widened exactly), every interpolation is the
same four fp64 operations in the same order, and the only sum is the 101-term trapezoid of terms <= 0.01, whose rounding in any
order is <= 100 * 2^-53 * 1 ~ 1e-14.  The tests print the measured maximum (on an MI355X: 0.0)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import det_eval_cases as DC
import det_eval_rule as DR
from hamer_yolo_amd import synth
from hamer_yolo_amd.yolo import metrics as M

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", "det_eval.npz"))
CASES = [str(c) for c in G["cases"]]
TOL = 1e-12


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def run_match(pred, pc, lab, lc, iouv=DC.IOUV):
    c, b, m = M.match_predictions(torch.from_numpy(pred).to(DEV), torch.from_numpy(pc).to(DEV), torch.from_numpy(lab).to(DEV),
                                  torch.from_numpy(lc).to(DEV), torch.from_numpy(iouv).to(DEV))
    assert c.is_cuda and c.dtype == torch.bool and b.dtype == torch.float32 and m.dtype == torch.int32
    return c.cpu().numpy(), b.cpu().numpy(), m.cpu().numpy()


def same_as_rule(pred, pc, lab, lc, iouv=DC.IOUV):
    c, b, m = run_match(pred, pc, lab, lc, iouv)
    rc, rb, rm = DR.match_batch(pred, pc, lab, lc, iouv)
    assert np.array_equal(c, rc.astype(bool)) and np.array_equal(m, rm) and np.array_equal(bits(b), bits(rb))
    return c, b, m


# ------------------------------------------------------------------ the match
def test_hand_worked_cases_in_one_batch():
    """Every hand-worked case as one image of one launch (NaN in the padding rows): the answers written down by hand, and
    the rule, exactly."""
    names = list(DC.HAND)
    imgs = [DC.hand_arrays(n)[:2] for n in names]
    pred, pc, lab, lc = DC.pack(imgs, 5, 4, fill=np.nan)
    c, b, m = same_as_rule(pred, pc, lab, lc)
    for i, n in enumerate(names):
        k = pc[i]
        DC.check_hand(n, c[i, :k], b[i, :k], m[i, :k])
        assert not c[i, k:].any() and (b[i, k:] == 0).all() and (m[i, k:] == -1).all()      # 0 / 0 / -1 past the count
    i = names.index("prefix_of_six")
    assert c[i, 0].tolist() == [True] * 6 + [False] * 4 and 0.76 < b[i, 0] < 0.78
    i = names.index("nan_pair")
    assert np.isnan(b[i, 1]) and b[i, 0] == 1.0


def test_one_by_one_alone():
    pred, lab = DC.hand_arrays("one_by_one")[:2]
    c, b, m = same_as_rule(*DC.pack([(pred, lab)], 1, 1))
    assert c.all() and m[0, 0] == 0 and b[0, 0] == 1.0


@pytest.mark.parametrize("n_pred,n_lab", [(70, 5), (3, 70)])
def test_counts_across_a_wave(n_pred, n_lab):
    rng = np.random.default_rng(n_pred)
    c, b, m = same_as_rule(*DC.pack([DC.random_image(rng, n_pred, n_lab)], n_pred, n_lab))
    assert n_pred < 64 or (m >= 0).sum() >= 2


def test_stride_300_counts_0_1_299_300():
    rng = np.random.default_rng(300)
    imgs = [DC.random_image(rng, n, 12) for n in (0, 1, 299, 300)]
    c, b, m = same_as_rule(*DC.pack(imgs, 300, 12, fill=np.nan))
    assert (m[0] == -1).all() and (m[2, 299] == -1) and (m[3] >= 0).sum() >= 6


def test_garbage_past_the_counts_and_clamped_counts():
    rng = np.random.default_rng(5)
    imgs = [DC.random_image(rng, 20, 6), DC.random_image(rng, 7, 9)]
    pred, pc, lab, lc = DC.pack(imgs, 32, 16, fill=np.nan)
    c, b, m = same_as_rule(pred, pc, lab, lc)
    assert not np.isnan(b).any()
    clean = DC.pack(imgs, 32, 16, fill=0.0)
    c0, b0, m0 = run_match(*clean)
    assert np.array_equal(c, c0) and np.array_equal(bits(b), bits(b0)) and np.array_equal(m, m0)
    # counts beyond the buffers are clamped to them, negative ones to 0 (the rows are zeros here, never garbage)
    same_as_rule(clean[0], np.array([1000, -5], np.int32), clean[2], np.array([-1, 4000], np.int32))


def test_niou_1_and_16():
    rng = np.random.default_rng(16)
    packed = DC.pack([DC.random_image(rng, 40, 10)], 40, 10)
    same_as_rule(*packed, iouv=np.array([0.5], np.float32))
    same_as_rule(*packed, iouv=np.linspace(0.2, 0.95, 16).astype(np.float32))


@pytest.fixture(scope="module")
def batch130():
    rng = np.random.default_rng(130)
    imgs = [DC.random_image(rng, int(rng.integers(0, 41)), int(rng.integers(0, 13))) for _ in range(130)]
    packed = DC.pack(imgs, 40, 12, fill=np.nan)
    return packed, run_match(*packed)


def test_130_images_in_one_launch(batch130):
    packed, (c, b, m) = batch130
    rc, rb, rm = DR.match_batch(*packed, DC.IOUV)
    assert np.array_equal(c, rc.astype(bool)) and np.array_equal(m, rm) and np.array_equal(bits(b), bits(rb))
    assert (m >= 0).sum() > 100


def test_batch_invariance(batch130):
    (pred, pc, lab, lc), (c, b, m) = batch130
    assert pc[13] > 0 and lc[13] > 0
    c1, b1, m1 = run_match(pred[13:14].copy(), pc[13:14].copy(), lab[13:14].copy(), lc[13:14].copy())
    assert c1.tobytes() == c[13:14].tobytes() and b1.tobytes() == b[13:14].tobytes() and m1.tobytes() == m[13:14].tobytes()


def test_numpy_in_numpy_out():
    rng = np.random.default_rng(8)
    pred, pc, lab, lc = DC.pack([DC.random_image(rng, 9, 4)], 9, 4)
    c, b, m = M.match_predictions(pred, pc, lab, lc)
    assert isinstance(c, np.ndarray) and c.dtype == bool and b.dtype == np.float32 and m.dtype == np.int32
    rc, rb, rm = DR.match_batch(pred, pc, lab, lc, DC.IOUV)
    assert np.array_equal(c, rc.astype(bool)) and np.array_equal(m, rm) and np.array_equal(bits(b), bits(rb))


# ------------------------------------------------------------------ AP
@pytest.mark.parametrize("v5", (False, True))
@pytest.mark.parametrize("P", (1, 2, 255, 256, 257, 1025, 70000))
def test_ap_against_the_rule(P, v5):
    tp, conf, pred_cls, target_cls = DC.ap_case(P, P)
    rap, rp, rr, uc = DR.ap_curves(tp, conf, pred_cls, target_cls, v5)
    order = np.argsort(-conf, kind="stable")
    x101, px = M._grids(torch.device(DEV))
    classes = torch.from_numpy(uc.astype(np.float32)).to(DEV)
    n_l = torch.from_numpy(np.array([(target_cls == c).sum() for c in uc], np.int32)).to(DEV)
    ap, p, r = M.ops.det_ap(torch.from_numpy(tp[order]).to(DEV), torch.from_numpy(conf[order]).to(DEV),
                            torch.from_numpy(pred_cls[order]).to(DEV), classes, n_l, x101, px, v5)
    d = [float(np.abs(a.cpu().numpy() - b).max()) for a, b in ((ap, rap), (p, rp), (r, rr))]
    print(f"P {P} v5 {int(v5)}: max |ap, p, r - rule| = {d[0]:.3g}, {d[1]:.3g}, {d[2]:.3g}")
    assert max(d) <= TOL


def test_p_zero_leaves_zeros():
    x101, px = M._grids(torch.device(DEV))
    e = torch.zeros(0, device=DEV)
    ap, p, r = M.ops.det_ap(torch.zeros(0, 10, dtype=torch.uint8, device=DEV), e, e, torch.tensor([0.0, 1.0], device=DEV),
                            torch.tensor([3, 4], dtype=torch.int32, device=DEV), x101, px)
    assert not ap.any() and not p.any() and not r.any()


@pytest.mark.parametrize("v5", (False, True))
@pytest.mark.parametrize("case", CASES)
def test_fixture_through_ap_per_class(case, v5):
    """The reference's recorded outputs through the public function, numpy in; the arg-max index equals the rule's."""
    tp, conf, pred_cls, target_cls = G[f"{case}/tp"], G[f"{case}/conf"], G[f"{case}/pred_cls"], G[f"{case}/target_cls"]
    p, r, ap, f1, cls = M.ap_per_class(tp.astype(bool), conf, pred_cls, target_cls, v5_metric=v5)
    k = f"{case}/v5_{int(v5)}"
    assert all(isinstance(a, np.ndarray) for a in (p, r, ap, f1, cls)) and cls.dtype == np.int32
    d = max(float(np.abs(a - G[f"{k}/{n}"]).max()) for n, a in (("p", p), ("r", r), ("ap", ap), ("f1", f1)))
    print(f"{case} v5 {int(v5)}: max distance from the reference's outputs {d:.3g}")
    assert d <= TOL and np.array_equal(cls, G[f"{k}/classes"])
    # the arg-max index is the rule's (the first maximum of f1.mean(0)), and the columns are the rule's columns there
    rap, rp, rr, uc = DR.ap_curves(tp, conf, pred_cls, target_cls, v5)
    i = DR.ap_per_class(tp, conf, pred_cls, target_cls, v5)[5]
    n_l = np.array([(target_cls == c).sum() for c in uc], np.int32)
    got_i = M._ap_device(torch.from_numpy(tp).to(DEV), torch.from_numpy(conf).to(DEV), torch.from_numpy(pred_cls).to(DEV),
                         torch.from_numpy(uc.astype(np.float32)).to(DEV), torch.from_numpy(n_l).to(DEV), v5)[4]
    assert int(got_i) == i
    assert np.abs(p - rp[:, i]).max() <= TOL and np.abs(r - rr[:, i]).max() <= TOL


@pytest.mark.parametrize("v5", (False, True))
@pytest.mark.parametrize("case", [str(c) for c in G["curves"]])
def test_fixture_through_compute_ap(case, v5):
    rec, pre = G[f"{case}/curve/recall"], G[f"{case}/curve/precision"]
    k = f"{case}/curve/v5_{int(v5)}"
    ap, mpre, mrec = M.compute_ap(rec, pre, v5_metric=v5)
    assert isinstance(ap, float) and abs(ap - float(G[k + "/ap"])) <= TOL
    assert np.array_equal(mpre, G[k + "/mpre"]) and np.array_equal(mrec, G[k + "/mrec"])
    dap, dmpre, dmrec = M.compute_ap(torch.from_numpy(rec).to(DEV), torch.from_numpy(pre).to(DEV), v5_metric=v5)
    assert dap.is_cuda and dap.shape == () and dmpre.is_cuda and float(dap) == ap and np.array_equal(dmrec.cpu().numpy(), mrec)


def test_compute_ap_long_curve():
    """More knots than threads: every thread owns a slice of the envelope."""
    rng = np.random.default_rng(9)
    tpv = rng.uniform(size=5000) < 0.4
    tpc, fpc = tpv.cumsum(), (~tpv).cumsum()
    rec, pre = tpc / (tpv.sum() + 7 + 1e-16), tpc / (tpc + fpc)
    for v5 in (False, True):
        ap, mpre, mrec = M.compute_ap(rec, pre, v5_metric=v5)
        rap, rmpre, rmrec = DR.compute_ap(rec, pre, v5)
        assert abs(ap - rap) <= TOL and np.array_equal(mpre, rmpre) and np.array_equal(mrec, rmrec)


def test_equal_confidences_follow_the_stable_order():
    tp, conf, pred_cls, target_cls = DC.ap_case(77, 400, ties=True)
    assert len(np.unique(conf)) < 10
    p, r, ap, f1, cls = M.ap_per_class(tp.astype(bool), conf, pred_cls, target_cls)
    rp, rr, rap, rf1, rcls, _ = DR.ap_per_class(tp, conf, pred_cls, target_cls)
    assert max(np.abs(p - rp).max(), np.abs(r - rr).max(), np.abs(ap - rap).max(), np.abs(f1 - rf1).max()) <= TOL
    # the order matters: the same predictions reversed give another curve
    rap2 = DR.ap_per_class(tp[::-1], conf[::-1], pred_cls[::-1], target_cls)[2]
    assert np.abs(rap2 - rap).max() > 1e-6


def test_device_tensors_in_device_tensors_out():
    tp, conf, pred_cls, target_cls = DC.ap_case(5, 300)
    out = M.ap_per_class(torch.from_numpy(tp).to(DEV), torch.from_numpy(conf).to(DEV), torch.from_numpy(pred_cls).to(DEV), target_cls)
    assert all(torch.is_tensor(o) and o.is_cuda for o in out) and out[4].dtype == torch.int32 and out[2].dtype == torch.float64
    out2 = M.ap_per_class(torch.from_numpy(tp).to(DEV), torch.from_numpy(conf).to(DEV), torch.from_numpy(pred_cls).to(DEV),
                          torch.from_numpy(target_cls).to(DEV))
    rule = DR.ap_per_class(tp, conf, pred_cls, target_cls)
    for o in (out, out2):
        for a, b in zip(o[:4], rule[:4]):
            assert np.abs(a.cpu().numpy() - b).max() <= TOL
        assert np.array_equal(o[4].cpu().numpy(), rule[4])


# ------------------------------------------------------------------ end to end
YOLO_SPEC = "synthetic:2:-2.2:0"      # the weights and frames of tests/test_gpu_yolo_f32.py: ~10 boxes per seeded 1080p frame
H, W = 1080, 1920


class _YCfg:
    weights = YOLO_SPEC; imgsz = 640; augment = True; conf_thres = 0.25; iou_thres = 0.35
    classes = [0, 1, 2]; agnostic_nms = True; device = "cuda"; save_path = "./output"


@pytest.fixture(scope="module")
def detected():
    """Four frames in two passes of two: per pass (dets (2 * 300, 6), count (2,)) as the plan holds them, cloned.  (The
    fp16 route finds 9, 11, 0 and 22 boxes: an image without predictions is among them.)"""
    from hamer_yolo_amd.yolo.detector import Detector
    det = Detector(_YCfg)
    passes = []
    for lo in (0, 2):
        frames = torch.stack([synth.frame_u8(H, W, seed=s) for s in (lo, lo + 1)]).to(DEV)
        p = det.engine.forward(list(frames))
        det.engine.nms_enqueue(p, _YCfg.conf_thres, _YCfg.iou_thres, _YCfg.classes, _YCfg.agnostic_nms, scale=True)
        passes.append((p["dets"].clone(), p["count"].clone()))
    counts = torch.cat([c for _, c in passes]).cpu().numpy()
    assert (counts > 0).sum() >= 3 and counts.sum() >= 8
    return det, passes


def _labels_from(dets, count, widen=None):
    """The predictions as labels (N, 300, 5) [cls, xyxy]; ``widen``: each box scaled about its centre by this factor."""
    d = dets.reshape(-1, 300, 6)
    box = d[:, :, :4].clone()
    if widen is not None:
        c, h = (box[:, :, :2] + box[:, :, 2:]) / 2, (box[:, :, 2:] - box[:, :, :2]) / 2 * widen
        box = torch.cat([c - h, c + h], 2)
    return torch.cat([d[:, :, 5:6], box], 2).contiguous(), count


def _nt(passes, nc=3):
    cls = torch.cat([d.reshape(-1, 300, 6)[i, :int(k), 5] for d, c in passes for i, k in enumerate(c.tolist())])
    return np.bincount(cls.cpu().numpy().astype(np.int64), minlength=nc)


def test_predictions_scored_against_themselves(detected):
    det, passes = detected
    ev = M.DetEvaluator(3)
    for dets, count in passes:
        c, b, m = ev(dets, count, *_labels_from(dets, count))
        assert c.is_cuda and b.is_cuda and m.is_cuda
    res = ev.result()
    nt = _nt(passes)
    assert res["seen"] == 4 and np.array_equal(res["nt"], nt) and np.array_equal(res["ap_class"], np.flatnonzero(nt))
    for k in ("mp", "mr", "map50", "map"):
        assert abs(res[k] - 1.0) <= TOL, (k, res[k])
    assert np.abs(res["ap"] - 1.0).max() <= TOL and np.abs(res["p"] - 1.0).max() <= TOL


def test_labels_at_iou_077(detected):
    """Each label is its prediction widened about its centre by 1 / sqrt(0.77): IoU 0.77, above the first six thresholds
    (0.5 .. 0.75) and below the seventh (0.8), so AP is 1 at six thresholds and 0 at four."""
    det, passes = detected
    ev = M.DetEvaluator(3)
    for dets, count in passes:
        lb, lc = _labels_from(dets, count, widen=1.0 / np.sqrt(0.77))
        c, b, m = ev(dets, count, lb, lc)
        for i, k in enumerate(count.tolist()):
            # boxes clipped at the frame border may be degenerate; the detector's boxes of these frames are not
            assert ((b[i, :k] > 0.76) & (b[i, :k] < 0.78)).all(), b[i, :k]
            assert (m[i, :k] == torch.arange(k, device=DEV)).all()
            assert c[i, :k, :6].all() and not c[i, :k, 6:].any()
    res = ev.result()
    assert abs(res["map50"] - 1.0) <= TOL and abs(res["map"] - 0.6) <= TOL and abs(res["mp"] - 1.0) <= TOL
    assert np.array_equal(res["nt"], _nt(passes))


def test_two_passes_equal_one(detected):
    det, passes = detected
    two, one = M.DetEvaluator(3), M.DetEvaluator(3)
    lab = [_labels_from(d, c, widen=1.0 / np.sqrt(0.77)) for d, c in passes]
    for (dets, count), (lb, lc) in zip(passes, lab):
        # drop the first label of every image: a false positive each, so the curves are not trivial
        two(dets, count, lb[:, 1:].contiguous(), (lc - 1).clamp(min=0))
    one(torch.cat([d for d, _ in passes]), torch.cat([c for _, c in passes]), torch.cat([l[:, 1:] for l, _ in lab]).contiguous(),
        (torch.cat([c for _, c in lab]) - 1).clamp(min=0))
    a, b = two.result(), one.result()
    assert a["seen"] == b["seen"] == 4 and a["nt"].sum() == sum(max(k - 1, 0) for _, c in passes for k in c.tolist())
    for k in ("mp", "mr", "map50", "map"):
        assert a[k] == b[k]
    for k in ("nt", "p", "r", "ap50", "ap", "ap_class"):
        assert np.array_equal(a[k], b[k])


def test_labels_without_predictions_count_and_nothing_correct_gives_zeros():
    ev = M.DetEvaluator(3)
    pred, lab = DC.hand_arrays("labels_no_predictions")[:2]
    ev(*DC.pack([(pred, lab)], 4, 4))
    z = ev.result()
    assert z["seen"] == 1 and z["mp"] == z["mr"] == z["map50"] == z["map"] == 0.0 and not z["nt"].any() and len(z["ap_class"]) == 0
    pred, lab = DC.hand_arrays("one_by_one")[:2]
    ev(*DC.pack([(pred, lab)], 4, 4))
    r = ev.result()
    assert r["seen"] == 2 and r["nt"].tolist() == [1, 2, 0] and r["ap_class"].tolist() == [0, 1]
    assert r["ap50"].tolist()[0] == 0.0 and abs(r["ap50"][1] - 0.5) < 0.01       # one of the two class-1 labels found: recall 0.5


@pytest.fixture(scope="module")
def folders(detected, tmp_path_factory):
    """pred/ and labels/ text files of the four frames (labels: the IoU-0.77 ones), and frames/ with the images."""
    from PIL import Image
    det, passes = detected
    root = tmp_path_factory.mktemp("det_eval")
    for sub in ("pred", "labels", "frames"):
        (root / sub).mkdir()
    i = 0
    for dets, count in passes:
        lb, _ = _labels_from(dets, count, widen=1.0 / np.sqrt(0.77))
        d = dets.reshape(-1, 300, 6).cpu().numpy()
        lb = lb.cpu().numpy()
        for k, n in enumerate(count.tolist()):
            M.save_label_file(str(root / "pred" / f"f{i}.txt"), d[k, :n], size=(W, H), conf=True)
            as_pred = np.concatenate([lb[k, :n, 1:5], np.ones((n, 1), np.float32), lb[k, :n, 0:1]], 1)
            M.save_label_file(str(root / "labels" / f"f{i}.txt"), as_pred, size=(W, H))
            Image.fromarray(synth.frame_u8(H, W, seed=i).numpy()[:, :, ::-1]).save(str(root / "frames" / f"f{i}.bmp"))
            i += 1
    return root


def test_score_folders(detected, folders):
    """%g keeps six digits: the IoUs move by ~1e-5 from 0.77, far from the thresholds 0.75 and 0.8, so the result is the same."""
    from hamer_yolo_amd import evaluate_det as E
    det, passes = detected
    (folders / "labels" / "orphan.txt").write_text("0 0.5 0.5 0.1 0.1\n")
    for size in (None, (W, H)):
        res = E.score_folders(str(folders / "pred"), str(folders / "labels"), size=size, nc=3)
        assert res["seen"] == 4 and res["nt"] == _nt(passes).tolist() and res["only_labels"] == ["orphan"]
        assert abs(res["map50"] - 1.0) <= TOL and abs(res["map"] - 0.6) <= TOL and abs(res["mp"] - 1.0) <= TOL
    (folders / "labels" / "orphan.txt").unlink()


def test_cli_on_a_tiny_folder(folders, tmp_path):
    out = tmp_path / "r.json"
    cmd = [sys.executable, "-m", "hamer_yolo_amd.evaluate_det", "--images", str(folders / "frames"), "--labels",
           str(folders / "labels"), "--weights", YOLO_SPEC, "--json", str(out), "--save-txt", str(tmp_path / "txt"), "--save-conf", "--det-frames", "2"]                              # the fixture's passes: two frames each
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads(out.read_text())
    assert res["seen"] == 4 and abs(res["map50"] - 1.0) <= TOL and abs(res["map"] - 0.6) <= TOL
    assert res["conf_thres"] == 0.25 and res["iou_thres"] == 0.35 and res["precise"] is False
    lines = r.stdout.splitlines()
    assert lines[0].split()[0] == "Class" and lines[1].split()[:3] == ["all", "4", str(res["labels"])] and "0.001 / 0.65" in r.stdout
    # the dumped predictions are the ones the pred/ folder holds
    for i in range(4):
        assert (tmp_path / "txt" / f"f{i}.txt").read_text() == (folders / "pred" / f"f{i}.txt").read_text()
