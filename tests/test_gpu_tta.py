"""GPU: the detector's test-time augmentation -- hm_tta_scale and hm_yolo_decode_batch_tta against the numpy rule
(tests/tta_rule.py), ``YoloEngine.forward(frames, tta=True)`` against the plain pass and against the oracle network
(oracle/yolo_ref) run per scale on torch's CPU scale_img, ``Detector(cfg, tta=True)`` against the oracle's box list, the
unchanged default, and ``evaluate_det.score_images`` with TTA.  The engine tests run at new_shape = 320 (a 540 x 960 frame
letterboxes to 192 x 320: scales of 192x320, 160x288 and 160x224, the last with 32 rows of pure padding).  Measured levels
are printed, appended as JSON lines to the file named by $HAMER_PARITY_REPORT when it is set, and recorded in DESIGN.md."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import tta_rule as TR
from hamer_yolo_amd import lib as L
from hamer_yolo_amd import ops, synth
from hamer_yolo_amd.yolo import arch, fuse
from hamer_yolo_amd.yolo import metrics as M
from hamer_yolo_amd.yolo.detector import Detector
from hamer_yolo_amd.yolo.engine import YoloEngine
from oracle import yolo_ref

pytestmark = pytest.mark.gpu

DEV = "cuda"
H, W = 540, 960                       # letterboxed to 192 x 320 at new_shape 320
N1, N_TTA = 3780, 8820                # rows of the plain pass and of the TTA pass (tests/test_tta_host.py)
DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
# fp32: four roundings of a convex combination of values in [0, 1]; 16-bit: one rounding of the type at 1.0 on top of it
TOL = {"f32": 1e-6, "f16": 2.0 ** -11 + 1e-6, "bf16": 2.0 ** -8 + 1e-6}


def _report(rep):
    print(json.dumps(rep))
    path = os.environ.get("HAMER_PARITY_REPORT")
    if not path:
        return
    try:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "a") as f:
            f.write(json.dumps(rep) + "\n")
    except OSError:
        pass


# ------------------------------------------------------------------ 1. hm_tta_scale
def _image(nb, h, w, dtype, seed):
    """(nb, h, w, 8): channels 0-2 a random permutation of k / n -- no two fp32 values alike, rounded to the type --
    channels 3-7 garbage the kernel must not carry over."""
    g = torch.Generator().manual_seed(seed)
    n = nb * h * w * 3
    x = torch.full((nb, h, w, 8), 0.75)
    x[..., :3] = (torch.randperm(n, generator=g).float() / float(n - 1)).reshape(nb, h, w, 3)
    return x.to(dtype)


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("flip", (False, True))
@pytest.mark.parametrize("ratio", (0.83, 0.67))
@pytest.mark.parametrize("hw", ((64, 96), (192, 320)))
@pytest.mark.parametrize("nb", (1, 3))
def test_tta_scale_equals_the_rule(nb, hw, ratio, flip, dt):
    dtype = DTYPES[dt]
    x = _image(nb, hw[0], hw[1], dtype, seed=hw[0] + nb)
    y = ops.tta_scale(x.to(DEV), ratio, 32, flip).cpu()
    sh, sw, hp, wp = TR.sizes(hw[0], hw[1], ratio)
    assert y.shape == (nb, hp, wp, 8) and y.dtype == dtype
    want = TR.scale_img(x[..., :3].permute(0, 3, 1, 2).double().numpy(), ratio, flip=flip)        # (nb, 3, hp, wp) float64
    got = y[..., :3].permute(0, 3, 1, 2).double().numpy()
    err = float(np.abs(got[:, :, :sh, :sw] - want[:, :, :sh, :sw]).max())
    assert err <= TOL[dt], err
    pad = torch.tensor(0.447, dtype=dtype)                                                       # the type's 0.447, exactly
    assert bool((y[:, sh:, :, :3] == pad).all()) and bool((y[:, :, sw:, :3] == pad).all())
    assert hp > sh or wp > sw
    assert bool((y[..., 3:] == 0).all())
    if flip:                                                                                     # = flip off on a mirrored input
        ym = ops.tta_scale(x.flip(2).contiguous().to(DEV), ratio, 32, False).cpu()
        assert torch.equal(ym.view(torch.uint8), y.view(torch.uint8))


@pytest.mark.parametrize("dt", list(DTYPES))
def test_tta_scale_half_size_has_no_padding(dt):
    """128 x 192 at ratio 0.5: 64 x 96, every output the mean of a 2 x 2 block (weights 0.5, 0.5), nothing padded."""
    dtype = DTYPES[dt]
    x = _image(2, 128, 192, dtype, seed=5)
    y = ops.tta_scale(x.to(DEV), 0.5).cpu()
    assert y.shape == (2, 64, 96, 8) and TR.sizes(128, 192, 0.5) == (64, 96, 64, 96)
    want = TR.scale_img(x[..., :3].permute(0, 3, 1, 2).double().numpy(), 0.5)
    got = y[..., :3].permute(0, 3, 1, 2).double().numpy()
    assert float(np.abs(got - want).max()) <= TOL[dt]
    blocks = x[..., :3].double().reshape(2, 64, 2, 96, 2, 3).mean((2, 4))
    assert float((y[..., :3].double() - blocks).abs().max()) <= TOL[dt]
    assert bool((y[..., 3:] == 0).all())


# ------------------------------------------------------------------ 2. the decode
@pytest.mark.parametrize("scale,flip", ((0.83, True), (0.67, False), (1.0, False), (0.67, True)))
def test_decode_tta_is_the_plain_decode_descaled_and_deflipped(scale, flip):
    lib = L.load()
    nb, nc, no, stride_rows, row0, full_w = 2, 3, 8, 200, 17, 320.0
    g = torch.Generator().manual_seed(3)
    sentinel = -777.0
    got = torch.full((nb * stride_rows, no), sentinel, device=DEV)
    plain = torch.full((nb * stride_rows, no), sentinel, device=DEV)
    r0 = row0
    written = torch.zeros(stride_rows, dtype=torch.bool)
    for (ny, nx), st, anc in (((5, 7), 8.0, arch.ANCHORS[0]), ((3, 4), 16.0, arch.ANCHORS[1])):
        raw = (torch.randn(nb * ny * nx, 3 * no, generator=g) * 2.0).to(DEV)
        a6 = (C.c_float * 6)(*[float(v) for v in anc])
        L.check(lib.hm_yolo_decode_batch(raw.data_ptr(), 3 * no, plain.data_ptr(), r0, ny, nx, nc, st, a6, nb, stride_rows,
                                         L.current_stream()), "hm_yolo_decode_batch")
        ops.yolo_decode_batch_tta(raw, got, r0, ny, nx, nc, st, anc, nb, stride_rows, scale, flip, full_w)
        written[r0:r0 + 3 * ny * nx] = True
        r0 += 3 * ny * nx
    torch.cuda.synchronize()
    assert r0 < stride_rows                                                # the per-image stride is larger than what was written
    got, plain = got.cpu().numpy().reshape(nb, stride_rows, no), plain.cpu().numpy().reshape(nb, stride_rows, no)
    w = written.numpy()
    want = plain.copy()
    want[:, w] = TR.descale(plain[:, w], scale, flip, full_w)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(got[:, w, 4:].view(np.uint32), plain[:, w, 4:].view(np.uint32))        # confidence and classes untouched
    assert np.all(got[:, ~w] == sentinel) and (~w).sum() == stride_rows - 3 * (35 + 12)
    if scale != 1.0:
        assert not np.array_equal(got[:, w, :4], plain[:, w, :4])


# ------------------------------------------------------------------ 3-5. the engine
@pytest.fixture(scope="module")
def frames():
    return [synth.frame_u8(H, W, seed=60 + i) for i in range(3)]


@pytest.fixture(scope="module")
def engine16():
    return YoloEngine(synth.yolo_state_dict(seed=0, nc=3), nc=3, device=DEV, new_shape=320)


@pytest.fixture(scope="module")
def engine32():
    return YoloEngine(synth.yolo_state_dict(seed=0, nc=3), nc=3, device=DEV, dtype=torch.float32, new_shape=320)


def _fused(seed=0, **kw):
    layers = arch.yolov7_layers()
    return layers, fuse.fuse_state_dict(synth.yolo_state_dict(seed=seed, nc=3, **kw), arch.conv_specs(layers, 3, 3))


@pytest.mark.parametrize("which", ("engine16", "engine32"))
def test_engine_tta_rows_batching_and_the_plain_pass_inside(which, frames, request):
    eng = request.getfixturevalue(which)
    two = [f.to(DEV) for f in frames[:2]]
    plain = eng.forward(two)
    torch.cuda.synchronize()
    assert plain["n_pred"] == N1 and "tta" not in plain
    ref = plain["pred"].clone()
    p = eng.forward(two, tta=True)
    torch.cuda.synchronize()
    assert p is not plain and p["n_pred"] == N_TTA == TR.n_rows(192, 320)[1] and p["pred"].shape == (2 * N_TTA, 8)
    assert [t["row0"] for t in p["tta"]] == [0, 3780, 3780 + 2835] and [(t["h"], t["w"]) for t in p["tta"]] == [(192, 320), (160, 288), (160, 224)]
    assert p["dets"].shape == (2 * 300, 6) and p["count"].shape == (2,)
    assert p["nms_ws"].numel() == eng.lib.hm_nms_workspace_bytes(N_TTA)
    pred = p["pred"].reshape(2, N_TTA, 8)
    assert bool(torch.isfinite(pred).all())
    for i in range(2):                                                     # the first n1 rows: the plain pass, bit for bit
        assert torch.equal(pred[i, :N1], ref[i * N1:(i + 1) * N1]), i
    assert torch.equal(eng.forward(two)["pred"], ref)                       # and the plain plan still gives its own bytes
    # three frames in one pass = three single passes
    three = [f.to(DEV) for f in frames]
    pb = eng.forward(three, tta=True)["pred"].clone().reshape(3, N_TTA, 8)
    for i, f in enumerate(three):
        assert torch.equal(eng.forward(f, tta=True)["pred"], pb[i]), i
    stacked = torch.stack(three)                                            # slices of one tensor: the one-launch letterbox
    assert torch.equal(eng.forward([stacked[i] for i in range(3)], tta=True)["pred"].reshape(3, N_TTA, 8), pb)
    # NMS takes the plan unchanged, per image or batched
    a = [d.clone() for d in eng.nms(eng.forward(three, tta=True), 0.001, 0.45, None, False)]
    b = eng.nms(eng.forward(three, tta=True), 0.001, 0.45, None, False, batched=True)
    assert len(a) == 3 and all(torch.equal(x, y) for x, y in zip(a, b)) and sum(len(x) for x in a) > 0


def _oracle_tta(layers, fused, frame, emu):
    """The oracle's TTA pred of one frame at new_shape 320: (pred (n_tta, 8), rows per scale)."""
    chw, g = yolo_ref.letterbox(frame.numpy(), new_shape=320)
    assert (g["out_h"], g["out_w"]) == (192, 320)
    x = (torch.from_numpy(chw).float() / 255.0)[None]
    if emu:
        x = x.half().float()                                               # the GPU branch resizes the half image (detector.py:110-125)
    with torch.no_grad():
        pred, rows = TR.oracle_pred(lambda xi: yolo_ref.yolo_forward(layers, fused, xi, 3, arch.ANCHORS, arch.STRIDES, emu=emu)[0], x)
    return pred[0], rows


@pytest.fixture(scope="module")
def oracle_f32(frames):
    torch.set_num_threads(max(1, min(16, len(os.sched_getaffinity(0)))))
    layers, fused = _fused()
    return [_oracle_tta(layers, fused, f, False) for f in frames[:2]]


@pytest.fixture(scope="module")
def oracle_f16(frames):
    torch.set_num_threads(max(1, min(16, len(os.sched_getaffinity(0)))))
    layers, fused = _fused()
    return [_oracle_tta(layers, fused, f, "fp16") for f in frames[:2]]


def test_fp32_route_tta_vs_the_fp32_oracle(engine32, frames, oracle_f32):
    """Per scale: yolo_ref.yolo_forward(emu=False) on torch's CPU scale_img of the oracle letterbox, de-scaled, de-flipped,
    concatenated.  Score columns within 1e-5 and xywh within 1e-2 letterbox px -- the bounds tests/test_gpu_yolo_f32.py
    holds the plain pass to -- and 1.5e-2 px on the de-scaled rows (dividing by 0.67 stretches a box error by 1.5).
    Measured on the MI355X, per scale: xywh 6.1e-4 / 6.1e-4 / 6.1e-4 px, scores 1.3e-6 / 8.9e-7 / 9.5e-7."""
    p = engine32.forward([f.to(DEV) for f in frames[:2]], tta=True)
    torch.cuda.synchronize()
    pred = p["pred"].cpu().reshape(2, N_TTA, 8)
    worst = [{"xywh": 0.0, "score": 0.0} for _ in TR.SCALES]
    for i, (ref, rows) in enumerate(oracle_f32):
        assert rows == [3780, 2835, 2205] and ref.shape == (N_TTA, 8)
        r0 = 0
        for k, n in enumerate(rows):
            d = (pred[i, r0:r0 + n] - ref[r0:r0 + n]).abs()
            worst[k]["xywh"] = max(worst[k]["xywh"], float(d[:, :4].max()))
            worst[k]["score"] = max(worst[k]["score"], float(d[:, 4:].max()))
            r0 += n
    _report({"test": "yolo_tta_fp32_pred_vs_fp32_oracle", "frames": 2, "scales": list(TR.SCALES),
             "max_xywh_px": [w["xywh"] for w in worst], "max_score": [w["score"] for w in worst]})
    for k, w in enumerate(worst):
        assert w["score"] <= 1e-5 and w["xywh"] <= (1e-2 if k == 0 else 1.5e-2), (k, w)


def test_fp16_route_tta_vs_the_fp16_oracle(engine16, frames, oracle_f16):
    """The same against emu="fp16" (the oracle resizes the half-rounded image, as the reference's GPU branch does), with the
    comparison tests/test_gpu_yolo.py applies to the plain pred: scores within 2e-2, xywh within 1.5e-1 of the box size
    (mean of w and h, at least 8 px) -- times 1.5 on the de-scaled rows.  Measured on the MI355X, per scale: xywh over size
    5.3e-3 / 3.0e-3 / 2.8e-3, scores 5.6e-4 / 5.1e-4 / 4.3e-4."""
    p = engine16.forward([f.to(DEV) for f in frames[:2]], tta=True)
    torch.cuda.synchronize()
    pred = p["pred"].cpu().reshape(2, N_TTA, 8)
    worst = [{"xywh_rel": 0.0, "score": 0.0} for _ in TR.SCALES]
    for i, (ref, rows) in enumerate(oracle_f16):
        r0 = 0
        for k, n in enumerate(rows):
            g, r = pred[i, r0:r0 + n], ref[r0:r0 + n]
            size = r[:, 2:4].abs().mean(1, keepdim=True).clamp_min(8.0)
            worst[k]["xywh_rel"] = max(worst[k]["xywh_rel"], float(((g[:, :4] - r[:, :4]).abs() / size).max()))
            worst[k]["score"] = max(worst[k]["score"], float((g[:, 4:] - r[:, 4:]).abs().max()))
            r0 += n
    _report({"test": "yolo_tta_fp16_pred_vs_fp16_oracle", "frames": 2, "scales": list(TR.SCALES),
             "max_xywh_over_size": [w["xywh_rel"] for w in worst], "max_score": [w["score"] for w in worst]})
    for k, w in enumerate(worst):
        assert w["score"] < 2e-2 and w["xywh_rel"] < (1.5e-1 if k == 0 else 1.5 * 1.5e-1), (k, w)


# ------------------------------------------------------------------ 6-7. the detector
YOLO_SPEC = "synthetic:2:-1.9:0"
# seeded 540 x 960 frames on which the ORACLE's TTA box list has 10, 15 and 9 boxes and 1 of its 136 unrounded corners lies
# within 0.02 px of a half-integer (found on the CPU; the plain pass gives 10, 14 and 7 boxes there)
DET_SEEDS = (3, 4, 7)


class _Cfg:
    weights = YOLO_SPEC; imgsz = 320; augment = True; conf_thres = 0.25; iou_thres = 0.35
    classes = [0, 1, 2]; agnostic_nms = True; device = "cuda"; save_path = "./output"


class _CfgTta(_Cfg):
    tta = True


@pytest.fixture(scope="module")
def det32_tta():
    return Detector(_Cfg, precise=True, tta=True)


def test_detector_tta_boxes_equal_the_oracles(det32_tta):
    """Detector(cfg, precise=True, tta=True).detect = the oracle TTA pred through non_max_suppression, scale_coords and
    round: count, order, labels, corners.  Exempt only a corner whose unrounded oracle value lies within 0.02 px of a
    half-integer (it may differ by 1), and such corners may number at most 5 % of all corners.  Measured on the MI355X:
    34 boxes, 136 corners equal, 1 eligible for the exemption, 0 used it."""
    torch.set_num_threads(max(1, min(16, len(os.sched_getaffinity(0)))))
    det = det32_tta
    assert det.tta is True and det.precise is True
    layers, fused = _fused(seed=2, obj_bias=-1.9, cls_bias=0.0)
    n_boxes = near_half = ties = 0
    singles, fr_dev = [], []
    for seed in DET_SEEDS:
        fr = synth.frame_u8(H, W, seed=seed)
        ref_pred, _ = _oracle_tta(layers, fused, fr, False)
        x = yolo_ref.non_max_suppression(ref_pred[None].clone(), 0.25, 0.35, [0, 1, 2], True)[0]
        unr = yolo_ref.scale_coords((192, 320), x[:, :4].clone(), fr.shape)
        assert len(x) >= 8, (seed, len(x))
        want = [['right' if c == 1 else 'left', b] for c, b in zip(x[:, 5].tolist(), unr.round().tolist())]
        half = [[abs(abs(float(u) - np.floor(float(u))) - 0.5) < 0.02 for u in row] for row in unr]
        near_half += int(sum(sum(r) for r in half))
        n_boxes += len(want)
        pred, got = det.detect(fr.numpy())
        singles.append((pred[0].cpu(), got[0]))
        fr_dev.append(fr.to(DEV))
        assert len(got[0]) == len(want), (seed, len(got[0]), len(want))
        assert torch.equal(pred[0][:, 5].cpu(), x[:, 5]), seed
        for j, ((lg, bg), (lw, bw)) in enumerate(zip(got[0], want)):
            assert lg == lw, (seed, j)
            for c in range(4):
                if bg[c] != bw[c]:
                    assert half[j][c] and abs(bg[c] - bw[c]) == 1.0, (seed, j, c, bg, bw, float(unr[j, c]))
                    ties += 1
    _report({"test": "yolo_tta_boxes_vs_fp32_oracle", "frames": len(DET_SEEDS), "boxes": n_boxes, "corner_ties_exempted": ties,
             "corners_within_0.02_of_half": near_half})
    assert near_half <= 0.05 * 4 * n_boxes and ties <= near_half
    preds, lists = det.detect_frames(fr_dev)                                # the batched calls: the single calls, bit for bit
    for (p1, l1), p2, l2 in zip(singles, preds, lists):
        assert torch.equal(p1, p2.cpu()) and l1 == l2
    p3, l3 = det.detect_frames_finish(det.detect_frames_enqueue(fr_dev))
    for (p1, l1), p2, l2 in zip(singles, p3, l3):
        assert torch.equal(p1, p2.cpu()) and l1 == l2


def test_default_is_unchanged_and_the_switches_are_read():
    """``augment = True`` in the config turns nothing on: Detector(cfg) and Detector(cfg, tta=False) give the same bytes, the
    plain pass's; config.tta is read when tta is None; TTA changes the result."""
    fr = synth.frame_u8(H, W, seed=4)
    a, b = Detector(_Cfg), Detector(_Cfg, tta=False)
    assert _Cfg.augment is True and a.tta is False and b.tta is False
    pa, la = a.detect(fr.numpy())
    pb, lb = b.detect(fr.numpy())
    assert torch.equal(pa[0], pb[0]) and la == lb and len(la[0]) > 0
    eng = a.engine
    p = eng.forward(fr.to(DEV))
    assert p["n_pred"] == N1 and torch.equal(eng.nms(p, 0.25, 0.35, [0, 1, 2], True), pa[0])
    assert [k for k in eng._plans if len(k) == 4] == []                     # no TTA plan was ever built
    c = Detector(_CfgTta)
    assert c.tta is True and Detector(_CfgTta, tta=False).tta is False
    pc, _ = c.detect(fr.numpy())
    assert c.engine._plan(H, W, 1, tta=True)["n_pred"] == N_TTA
    mine = yolo_ref.non_max_suppression(c.engine._plan(H, W, 1, tta=True)["pred"].cpu()[None], 0.25, 0.35, [0, 1, 2], True)[0]
    mine[:, :4] = yolo_ref.scale_coords((192, 320), mine[:, :4], fr.shape).round()
    assert torch.equal(pc[0].cpu(), mine)                                   # the oracle's NMS on the GPU's own TTA pred


# ------------------------------------------------------------------ 8. evaluate_det
def test_score_images_with_tta(tmp_path):
    from PIL import Image
    from hamer_yolo_amd import evaluate_det as E
    det = Detector(_Cfg, tta=True)
    (tmp_path / "frames").mkdir()
    (tmp_path / "labels").mkdir()
    frs = [synth.frame_u8(H, W, seed=s) for s in DET_SEEDS]
    for i, fr in enumerate(frs):
        Image.fromarray(fr.numpy()[:, :, ::-1]).save(str(tmp_path / "frames" / f"f{i}.bmp"))
        boxes, _ = det.detect(fr.numpy())
        rows = boxes[0].cpu().numpy()[::2]                                  # every other detection is a label, the rest false positives
        lab = np.concatenate([rows[:, :4], np.ones((len(rows), 1), np.float32), rows[:, 5:6]], 1)
        M.save_label_file(str(tmp_path / "labels" / f"f{i}.txt"), lab, size=(W, H))
    res = E.score_images(str(tmp_path / "frames"), str(tmp_path / "labels"), det, det_frames=2)
    assert res["augment"] is True and res["seen"] == 3 and res["labels"] > 0
    ev = M.DetEvaluator(3)
    for chunk in ((0, 1), (2,)):                                             # the passes det_frames=2 makes of three frames
        p = det.engine.forward([frs[i].to(DEV) for i in chunk], tta=True)
        det.engine.nms_enqueue(p, 0.25, 0.35, [0, 1, 2], True, scale=True)
        T = [M.load_label_file(str(tmp_path / "labels" / f"f{i}.txt")) for i in chunk]
        for t in T:
            t[:, 1:5] *= np.array([W, H, W, H], np.float32)
        lb, lc = E._pack(T, 5, max(len(t) for t in T))
        ev(p["dets"], p["count"], lb, lc)
    want = E._result_dict(ev.result(), list(det.engine.names), {})
    for k in ("seen", "labels", "nt", "mp", "mr", "map50", "map", "classes"):
        assert res[k] == want[k], k
    assert 0.0 < res["map50"] <= 1.0
    plain = E.score_images(str(tmp_path / "frames"), str(tmp_path / "labels"), Detector(_Cfg), det_frames=2)
    assert plain["augment"] is False
