"""GPU: hm_yolo_nms_batch against the shipped per-image kernel (same bytes), against the numpy rule (tests/nms_rule.py, which
equals the reference's recorded outputs, tests/test_nms_batch_host.py) in multi-label mode and on the large paths, through
YoloEngine.nms / general.non_max_suppression, and through ``evaluate_det --protocol test``.

Every comparison of boxes is exact (``torch.equal`` / ``np.array_equal``): the kernel and the rule run the same single IEEE
fp32 operations in the same order, and the order of the candidates is a total order (score, then row * nc + class)."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import nms_rule as NR
from hamer_yolo_amd import lib as L
from hamer_yolo_amd import synth

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", "nms_multi.npz"))
SENTINEL = -12345.0


def letterbox_plan(h=1080, w=1920):
    lp = L.LetterboxPlan()
    L.check(L.load().hm_letterbox_plan_make(h, w, 640, 32, C.byref(lp)), "hm_letterbox_plan_make")
    return lp


def plan_tuple(lp):
    return (lp.pad_x, lp.pad_y, lp.gain, lp.src_w, lp.src_h)


def run_batch(pred, conf, iou, classes=None, agnostic=False, multi_label=False, lp=None, gap=0, dets_stride=300, max_det=300):
    """pred (nb, n, 5+nc) numpy -> (list of (k, 6) numpy, the untouched-rows check done).  ``gap``: floats between images."""
    lib = L.load()
    nb, n, no = pred.shape
    stride = n * no + gap
    buf = torch.full((nb, stride), float("nan"), dtype=torch.float32, device=DEV)
    buf[:, :n * no] = torch.from_numpy(pred.reshape(nb, -1)).to(DEV)
    ws = torch.empty(lib.hm_nms_batch_workspace_bytes(nb, n, no - 5, int(multi_label)), dtype=torch.uint8, device=DEV)
    dets = torch.full((nb, dets_stride, 6), SENTINEL, dtype=torch.float32, device=DEV)
    count = torch.full((nb,), -1, dtype=torch.int32, device=DEV)
    L.check(lib.hm_yolo_nms_batch(buf.data_ptr(), stride, nb, n, no - 5, conf, iou, NR.class_mask(classes), int(agnostic), int(multi_label),
                                  max_det, C.byref(lp) if lp is not None else None, dets.data_ptr(), dets_stride, count.data_ptr(),
                                  ws.data_ptr(), ws.numel(), L.current_stream()), "hm_yolo_nms_batch")
    counts = count.tolist()
    dets = dets.cpu()
    for i, k in enumerate(counts):
        assert 0 <= k <= max_det and (dets[i, k:] == SENTINEL).all(), "rows past count[i] must not be written"
    return [dets[i, :k].numpy() for i, k in enumerate(counts)]


def run_single(pred_image, conf, iou, classes, agnostic, lp):
    lib = L.load()
    n, no = pred_image.shape
    x = torch.from_numpy(np.ascontiguousarray(pred_image)).to(DEV)
    ws = torch.empty(lib.hm_nms_workspace_bytes(n), dtype=torch.uint8, device=DEV)
    dets = torch.full((300, 6), SENTINEL, dtype=torch.float32, device=DEV)
    count = torch.full((1,), -1, dtype=torch.int32, device=DEV)
    L.check(lib.hm_yolo_nms(x.data_ptr(), n, no - 5, conf, iou, NR.class_mask(classes), int(agnostic), 300,
                            C.byref(lp) if lp is not None else None, dets.data_ptr(), count.data_ptr(), ws.data_ptr(), ws.numel(),
                            L.current_stream()), "hm_yolo_nms")
    return dets[:int(count.item())].cpu().numpy()


def same(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ------------------------------------------------------------------ (a) the shipped kernel's bytes
@pytest.mark.parametrize("with_plan", (False, True))
@pytest.mark.parametrize("agnostic,classes", ((1, [0, 1, 2]), (0, [0, 1])))
def test_best_class_is_the_shipped_kernel_byte_for_byte(agnostic, classes, with_plan):
    pred = NR.pass_nc3(5, 5, 600, ties=40)
    lp = letterbox_plan() if with_plan else None
    assert not (pred[1, :, 4] > 0.25).any() and (pred[2, :, 5:] * pred[2, :, 4:5] > 0.25).all()
    s0 = pred[0, :, 5:] * pred[0, :, 4:5]
    assert (s0[1:] == s0[:-1]).all(1).sum() >= 30                                     # equal scores in neighbouring rows
    got = run_batch(pred, 0.25, 0.35, classes, agnostic, False, lp, gap=24, dets_stride=320)
    want = [run_single(pred[i], 0.25, 0.35, classes, agnostic, lp) for i in range(5)]
    assert [len(g) for g in got] == [len(w) for w in want] and len(got[1]) == 0 and min(len(got[i]) for i in (0, 2, 3, 4)) > 20
    for g, w in zip(got, want):
        assert same(g, w)
    rule = NR.nms(pred, 0.25, 0.35, classes, agnostic, False, plan=None if lp is None else plan_tuple(lp))
    assert all(same(g, r) for g, r in zip(got, rule))


# ------------------------------------------------------------------ (b) multi-label
@pytest.mark.parametrize("agnostic", (0, 1))
def test_multi_label_equals_the_rule(agnostic):
    pred = NR.pass_nc3(6, 4, 400, ties=30)
    got = run_batch(pred, 0.001, 0.65, None, agnostic, True)
    want = NR.nms(pred, 0.001, 0.65, None, agnostic, True)
    print("kept", [len(g) for g in got])
    assert len(got[1]) == 0 and len(got[0]) > 100
    assert all(same(g, w) for g, w in zip(got, want))
    # a tie was decided inside the kept rows: two kept candidates with one score, the lower row * nc + class first
    assert any((g[1:, 4] == g[:-1, 4]).any() for g in got)
    best = run_batch(pred, 0.001, 0.65, None, agnostic, False)
    # class-aware, a second label of a box survives; agnostic, it has IoU 1 with the first and never does
    assert all(same(g, b) for g, b in zip(got, best)) if agnostic else any(not same(g, b) for g, b in zip(got, best))


def test_multi_label_with_one_class_is_best_class():
    pred = np.stack([NR.make_image(np.random.default_rng(7), 400, 1, ties=20), NR.make_image(np.random.default_rng(8), 400, 1)])
    a, b = run_batch(pred, 0.001, 0.65, None, 0, True), run_batch(pred, 0.001, 0.65, None, 0, False)
    want = NR.nms(pred, 0.001, 0.65, None, 0, True)
    assert all(same(x, y) and same(x, w) for x, y, w in zip(a, b, want)) and len(a[0]) > 50
    fx = run_batch(G["pred/b"], 0.001, 0.65, None, 0, True)
    assert same(fx[0], G["nc1_multi/out0"])


@pytest.mark.parametrize("case", [str(c) for c in G["cases"] if str(c).startswith(("nc3/ml1", "ties/"))])
def test_fixture_cases(case):
    """The reference's recorded outputs, straight from the kernel."""
    cl = G[f"{case}/classes"]
    got = run_batch(G[f"pred/{str(G[f'{case}/pred'])}"], float(G[f"{case}/conf"]), float(G[f"{case}/iou"]), None if cl.size == 0 else cl.tolist(),
                    bool(G[f"{case}/agnostic"]), bool(G[f"{case}/multi_label"]))
    assert [len(g) for g in got] == G[f"{case}/count"].tolist()
    assert all(same(g, G[f"{case}/out{i}"]) for i, g in enumerate(got))


# ------------------------------------------------------------------ (c) the large paths
def test_workspace_sort_truncation_and_both_loop_ends():
    """nb = 2, nc = 32, multi-label, conf 0.001.  Image 0: 32000 candidates (> 16384: sorted in the workspace; > 30000: cut),
    spread boxes, the max_det cap ends the loop.  Image 1: ~17000 candidates in four clusters, fewer than 300 kept, the loop
    walks every candidate."""
    pred = np.stack([NR.image_truncated(), NR.image_crowded()])
    ncand = [int((p[:, 5:] * p[:, 4:5] > np.float32(0.001)).sum()) for p in pred]
    assert ncand[0] == 32000 and 16384 < ncand[1] < 18000, ncand
    got = run_batch(pred, 0.001, 0.65, None, 0, True)
    want = NR.nms(pred, 0.001, 0.65, None, 0, True)
    print("candidates", ncand, "kept", [len(g) for g in got])
    assert len(got[0]) == 300 and 32 <= len(got[1]) < 300
    assert same(got[0], want[0]) and same(got[1], want[1])
    assert same(got[0], G["nc32_cut/out0"])
    # max_det at the other end of its range
    full = run_batch(pred[:1], 0.001, 0.65, None, 0, True, max_det=1024, dets_stride=1024)[0]
    assert len(full) == 1024 and same(full, NR.nms(pred[:1], 0.001, 0.65, None, 0, True, max_det=1024)[0])


def test_the_30000_cut_decides_the_result():
    """Best-class mode, one class, 31000 survivors: 30200 boxes in four tight clusters hold the best scores, 800 isolated boxes
    the worst.  The cut leaves 30000 clustered candidates, so a handful is kept; without it the isolated boxes would fill the
    300.  Scores are distinct, so no tie sits on the cut."""
    rng = np.random.default_rng(9)
    crowd = NR.make_image(rng, 30200, 1, extent=(640.0, 640.0), clusters=4)
    crowd[:, 4] = 0.5 + rng.permutation(30200).astype(np.float32) / 30200 * 0.4
    lone = np.zeros((800, 6), np.float32)
    k = np.arange(800)
    lone[:, 0], lone[:, 1], lone[:, 2:4] = 1000 + (k % 40) * 30, 1000 + (k // 40) * 30, 16
    lone[:, 4] = 0.01 + rng.permutation(800).astype(np.float32) / 800 * 0.05
    p = np.concatenate([crowd, lone])[rng.permutation(31000)][None]
    p[0, :, 5] = 1.0
    got = run_batch(p, 0.001, 0.65, None, 0, False)[0]
    print("kept", len(got))
    assert 4 <= len(got) < 40 and (got[:, 4] >= 0.5).all() and same(got, NR.nms(p, 0.001, 0.65)[0])


# ------------------------------------------------------------------ (d) engine, (e) driver
YOLO_SPEC = "synthetic:2:-2.2:0"      # the weights of tests/test_gpu_det_eval.py


class _YCfg:
    weights = YOLO_SPEC; imgsz = 640; augment = True; conf_thres = 0.25; iou_thres = 0.35
    classes = [0, 1, 2]; agnostic_nms = True; device = "cuda"; save_path = "./output"


@pytest.fixture(scope="module")
def detector():
    from hamer_yolo_amd.yolo.detector import Detector
    return Detector(_YCfg)


def test_engine_batched_and_multi_label(detector):
    from hamer_yolo_amd.yolo import general
    eng = detector.engine
    frames = torch.stack([synth.frame_u8(540, 960, seed=s) for s in (0, 1, 2)]).to(DEV)
    p = eng.forward(list(frames))
    assert p["nb"] == 3 and p["n_pred"] == 15120 and "nms_batch_ws" not in p
    loop = eng.nms(p, 0.25, 0.35, [0, 1, 2], True)
    assert "nms_batch_ws" not in p                                                      # the default path allocates nothing new
    p["dets"].fill_(SENTINEL)
    batched = eng.nms(p, 0.25, 0.35, [0, 1, 2], True, batched=True)
    assert sum(len(d) for d in loop) > 3 and all(torch.equal(a, b) for a, b in zip(loop, batched))
    assert list(p["nms_batch_ws"]) == [0]
    pred = p["pred"].reshape(3, 15120, -1).clone()
    want = NR.nms(pred.cpu().numpy(), 0.001, 0.65, None, False, True)
    multi = eng.nms(p, 0.001, 0.65, None, False, multi_label=True)
    assert sorted(p["nms_batch_ws"]) == [0, 1]
    plan = plan_tuple(p["lp"])
    print("kept", [len(m) for m in multi], "deployed", [len(d) for d in loop])
    assert all(same(m.cpu().numpy(), NR.scale(w, plan)) for m, w in zip(multi, want))
    assert all(len(m) > len(d) for m, d in zip(multi, loop))
    out = general.non_max_suppression(pred, 0.001, 0.65, multi_label=True)
    assert all(o.is_cuda and same(o.cpu().numpy(), w) for o, w in zip(out, want))
    host = general.non_max_suppression(pred[:1].cpu(), 0.25, 0.45, classes=[0, 2])       # a host tensor is uploaded
    assert host[0].is_cuda and same(host[0].cpu().numpy(), NR.nms(pred[:1].cpu().numpy(), 0.25, 0.45, [0, 2])[0])


H, W = 1080, 1920
TOL = 1e-12                            # the bound tests/test_gpu_det_eval.py holds its own text round trip to


@pytest.fixture(scope="module")
def folder(detector, tmp_path_factory):
    """frames/ with four seeded 1080p frames and labels/ made as tests/test_gpu_det_eval.py makes them: every deployed
    prediction widened about its centre by 1 / sqrt(0.77).  Returns (root, deployed counts)."""
    from PIL import Image
    from hamer_yolo_amd.yolo import metrics as M
    root = tmp_path_factory.mktemp("nms_batch_eval")
    (root / "frames").mkdir(); (root / "labels").mkdir()
    counts = []
    for lo in (0, 2):
        frames = torch.stack([synth.frame_u8(H, W, seed=s) for s in (lo, lo + 1)]).to(DEV)
        p = detector.engine.forward(list(frames))
        dets = detector.engine.nms(p, _YCfg.conf_thres, _YCfg.iou_thres, _YCfg.classes, _YCfg.agnostic_nms)
        for k, d in enumerate(dets):
            d = d.cpu().numpy()
            c, h = (d[:, :2] + d[:, 2:4]) / 2, (d[:, 2:4] - d[:, :2]) / 2 * np.float32(1.0 / np.sqrt(0.77))
            lab = np.concatenate([c - h, c + h, np.ones((len(d), 1), np.float32), d[:, 5:6]], 1).astype(np.float32)
            M.save_label_file(str(root / "labels" / f"f{lo + k}.txt"), lab, size=(W, H))
            Image.fromarray(synth.frame_u8(H, W, seed=lo + k).numpy()[:, :, ::-1]).save(str(root / "frames" / f"f{lo + k}.bmp"))
            counts.append(len(d))
    return root, counts


def test_driver_protocol_test(folder, tmp_path):
    from hamer_yolo_amd import evaluate_det as E
    root, deployed = folder
    out, txt = tmp_path / "r.json", tmp_path / "txt"
    cmd = [sys.executable, "-m", "hamer_yolo_amd.evaluate_det", "--images", str(root / "frames"), "--labels", str(root / "labels"),
           "--weights", YOLO_SPEC, "--protocol", "test", "--save-txt", str(txt), "--save-conf", "--json", str(out), "--det-frames", "2"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads(out.read_text())
    assert res["protocol"] == "test" and res["conf_thres"] == 0.001 and res["iou_thres"] == 0.65
    assert res["multi_label"] is True and res["agnostic"] is False and res["seen"] == 4
    assert "protocol test" in r.stdout and "multi-label" in r.stdout and "class-aware" in r.stdout and "--save-hybrid" in r.stdout
    lines = [len((txt / f"f{i}.txt").read_text().splitlines()) for i in range(4)]
    print("predictions per image: test", lines, "deployed", deployed)
    assert all(n <= 300 for n in lines) and any(a > b for a, b in zip(lines, deployed))
    again = E.score_folders(str(txt), str(root / "labels"), size=(W, H), nc=3)
    print("json map50 %.15g map %.15g; text round trip map50 %.15g map %.15g" % (res["map50"], res["map"], again["map50"], again["map"]))
    assert again["seen"] == res["seen"] and again["nt"] == res["nt"]
    assert abs(again["map50"] - res["map50"]) <= TOL and abs(again["map"] - res["map"]) <= TOL
