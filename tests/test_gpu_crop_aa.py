"""GPU: the anti-aliased HaMeR crop (csrc/crop_aa.hip: hm_crop_batch_aa; hamer_inference.prepare_item and the ``antialias``
switch) against the fp64 rule of tests/crop_aa_rule.py.

The bound is not a number chosen in advance: the rule is evaluated in fp64 (the truth) and in plain numpy fp32 on the blurred
cases of this file, ``d_cpu`` is the largest distance between the two, and the kernel has to stay within ``4 x d_cpu`` of the
truth.  Another fp32 summation order costs about 1.4 x d_cpu; a misplaced or mis-weighted tap shows at 1e-2 or more, so the
factor hides none.  Every test prints its figures before it asserts."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import crop_aa_rule as R  # noqa: E402

from hamer_yolo_amd import infer, ops  # noqa: E402
from hamer_yolo_amd.infer import hamer_inference, hand_record, process_batch_manopara  # noqa: E402
from oracle import crop_ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
P = 256
MEAN = 255.0 * np.array([0.485, 0.456, 0.406])
STD = 255.0 * np.array([0.229, 0.224, 0.225])

# 480 x 640: the 8-bit path, the float path without blur, half outside the frame, a negative corner, r = 2, r = 4, and the whole
# frame with its replicated edges inside the crop
SEVEN = [[250, 170, 390, 310], [230, 150, 410, 330], [500, 300, 700, 560], [-60, -40, 180, 200], [170, 120, 470, 360],
         [100, 60, 540, 400], [0, 0, 640, 480]]
SEVEN = [["right" if i % 2 == 0 else "left", [float(v) for v in b]] for i, b in enumerate(SEVEN)]
SEVEN_S_R = [(467, None), (600, 0), (667, 1), (800, 1), (1000, 2), (1467, 4), (2133, 6)]
# 1080 x 1920: r = 18, and r = 6 with about half of the crop inside the frame
LARGE = [["right", [200.0, 100.0, 1700.0, 1000.0]], ["left", [700.0, 300.0, 1300.0, 900.0]]]
LARGE_S_R = [(5000, 18), (2000, 6)]


def _noise(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def _scalars(bboxs):
    out = []
    for label, (x1, y1, x2, y2) in bboxs:
        cx, cy, S = crop_ref.bbox_to_center_size(x1, y1, x2, y2)
        out.append((cx, cy, S, label != "right"))
    return out


def _gpu_crop(frame, bboxs, out=None):
    rec = ops.crop_boxes_aa(_scalars(bboxs), P).to(DEV)
    return ops.crop_batch_aa(torch.from_numpy(frame).to(DEV), rec, MEAN, STD, P, out=out)


@pytest.fixture(scope="module")
def cases():
    """The two noise frames, their hands, the truth and the fp32 rule, computed once; ``bound`` = 4 x d_cpu."""
    c = {"small": (_noise(480, 640, 11), SEVEN, SEVEN_S_R), "large": (_noise(1080, 1920, 12), LARGE, LARGE_S_R)}
    out, d_cpu = {}, 0.0
    for name, (frame, bboxs, s_r) in c.items():
        for bbox, (S, r) in zip(bboxs, s_r):                       # the cases are the ones the docstrings name
            got = crop_ref.bbox_to_center_size(*bbox[1])[2]
            blur = R.blur_of_size(got, P)
            assert round(got) == S and (blur[1] if blur else None) == r, (bbox, got, blur)
        truth = R.prepare_items(frame, bboxs, MEAN, STD)
        f32 = R.prepare_items(frame, bboxs, MEAN, STD, dtype=np.float32)
        blurred = [i for i, b in enumerate(bboxs) if R.is_blurred(b)]
        d = [float(np.abs(f32[i].astype(np.float64) - truth[i]).max()) for i in blurred]
        print(f"[crop_aa] {name}: d_cpu per blurred hand {['%.2e' % v for v in d]}")
        d_cpu = max([d_cpu] + d)
        out[name] = {"frame": frame, "bboxs": bboxs, "truth": truth, "blurred": blurred}
    out["d_cpu"], out["bound"] = d_cpu, 4.0 * d_cpu
    print(f"[crop_aa] d_cpu {d_cpu:.3e}, bound {out['bound']:.3e}")
    assert 1e-7 < d_cpu < 2e-6                       # fp32 arithmetic on values of a few units: a few ulp, nothing else
    return out


def test_aa_crop_matches_rule(cases):
    c = cases["small"]
    got = _gpu_crop(c["frame"], c["bboxs"]).cpu().numpy()
    plain = ops.crop_batch(torch.from_numpy(c["frame"]).to(DEV), ops.crop_boxes(_scalars(c["bboxs"]), P).to(DEV), MEAN, STD, P).cpu().numpy()
    assert c["blurred"] == [1, 2, 3, 4, 5, 6]
    assert np.array_equal(got[0], plain[0])                                   # df <= 1.1: hm_crop_batch's bytes
    assert np.array_equal(got[0], c["truth"][0].astype(np.float32))
    for i in c["blurred"]:
        d = float(np.abs(got[i].astype(np.float64) - c["truth"][i]).max())
        away = float(np.abs(plain[i].astype(np.float64) - c["truth"][i]).max())
        print(f"[crop_aa] hand {i} S {SEVEN_S_R[i][0]} r {SEVEN_S_R[i][1]}: |gpu - fp64| {d:.3e} (bound {cases['bound']:.3e}); "
              f"the unfiltered crop is {away:.3g} away")
        assert d <= cases["bound"], (i, d)
    assert float(np.abs(plain[4].astype(np.float64) - c["truth"][4]).max()) > 0.5       # (the prefilter is no small change)


def test_large_radius(cases):
    c = cases["large"]
    got = _gpu_crop(c["frame"], c["bboxs"]).cpu().numpy()
    H, W = c["frame"].shape[:2]
    cx, cy, S = crop_ref.bbox_to_center_size(*c["bboxs"][1][1])
    inside = (max(0.0, min(W, cx + S / 2) - max(0.0, cx - S / 2)) * max(0.0, min(H, cy + S / 2) - max(0.0, cy - S / 2))) / (S * S)
    assert 0.45 < inside < 0.6
    for i in (0, 1):
        d = float(np.abs(got[i].astype(np.float64) - c["truth"][i]).max())
        print(f"[crop_aa] large hand {i} S {LARGE_S_R[i][0]} r {LARGE_S_R[i][1]}: |gpu - fp64| {d:.3e} (bound {cases['bound']:.3e})")
        assert d <= cases["bound"], (i, d)


def test_ramp_known_answer(cases):
    """Independent of scipy: a Gaussian with symmetric normalised taps leaves a linear ramp as it is away from the edges, so
    wherever the taps and their support are interior the output is the ramp at the source coordinate."""
    n = 128
    yy, xx = np.mgrid[0:n, 0:n]
    frame = np.stack([xx + yy, 2 * xx, yy + 100], axis=-1).astype(np.uint8)          # B, G, R planes; all within 0 .. 254
    assert int((np.stack([xx + yy, 2 * xx, yy + 100], axis=-1)).max()) <= 255
    bboxs = [["right", [-56.0, -56.0, 184.0, 184.0]], ["left", [-156.0, -156.0, 284.0, 284.0]], ["right", [-150.0, -170.0, 290.0, 270.0]]]
    got = _gpu_crop(frame, bboxs).cpu().numpy().astype(np.float64)
    mean, std = np.float32(MEAN).astype(np.float64), np.float32(STD).astype(np.float64)
    for i, (bbox, want_r) in enumerate(zip(bboxs, (1, 4, 4))):
        cx, cy, S = crop_ref.bbox_to_center_size(*bbox[1])
        assert R.blur_of_size(S, P)[1] == want_r
        M = crop_ref.gen_trans_from_patch(cx, cy, S, S, P, P)
        sx, sy, fx, fy = R.warp_coords(M, P, P)
        x, y = sx + fx / 32.0, sy + fy / 32.0
        want = np.stack([(y + 100 - mean[0]) / std[0], (2 * x - mean[1]) / std[1], (x + y - mean[2]) / std[2]])      # R, G, B
        inside = R.interior_mask(M, P, P, n, n, want_r)
        if bbox[0] != "right":
            want, inside = want[:, :, ::-1], inside[:, ::-1]
        d = float(np.abs(got[i] - want)[:, inside].max())
        print(f"[crop_aa] ramp hand {i} r {want_r}: {int(inside.sum())} interior pixels, max distance {d:.3e} (bound {cases['bound']:.3e})")
        assert inside.sum() >= 300 and d <= cases["bound"]


def test_batch_position_independence(cases):
    c = cases["small"]
    hand = c["bboxs"][5]                                                                 # S = 1467, r = 4, a left hand
    others = [b for i, b in enumerate(c["bboxs"]) if i != 5]
    alone = _gpu_crop(c["frame"], [hand])
    first = _gpu_crop(c["frame"], [hand] + others)
    last = _gpu_crop(c["frame"], others + [hand])
    big = torch.full((9, 3, P, P), -7.0, device=DEV)
    _gpu_crop(c["frame"], others[:2] + [hand], out=big[4:7])
    torch.cuda.synchronize()
    assert torch.equal(first[0], alone[0]) and torch.equal(last[6], alone[0]) and torch.equal(big[6], alone[0])
    assert bool((big[:4] == -7.0).all()) and bool((big[7:] == -7.0).all())               # nothing outside the slice is written
    assert torch.equal(big[4], first[1]) and torch.equal(last[0], first[1])


# ---------------------------------------------------------------------------------------------------------- the Python surface
class _Cfg:
    ckpt_path = "synthetic:0"
    model_cfg = None
    use_onnx = False
    onnx_path = None


class _CfgAA(_Cfg):
    antialias = True


@pytest.fixture(scope="module")
def hi():
    h = hamer_inference(_Cfg)
    assert h.antialias is False and h.precise is False
    return h


@pytest.fixture(scope="module")
def hi_aa(hi):
    """hamer_inference(cfg, antialias=True) over the SAME synthetic model (the constructor runs; the weights are not built twice)."""
    real = infer.load_hamer
    infer.load_hamer = lambda *a, **k: (hi.model, hi.cfg)
    try:
        h = hamer_inference(_Cfg, antialias=True)
        assert h.antialias is True and h.precise is False
        assert hamer_inference(_CfgAA).antialias is True and hamer_inference(_CfgAA, antialias=False).antialias is False
        assert hamer_inference(_CfgAA, precise=False).antialias is True                  # the two switches do not touch each other
    finally:
        infer.load_hamer = real
    return h


def test_prepare_item_and_switch(cases, hi, hi_aa):
    c = cases["small"]
    frame = c["frame"]
    dets = [c["bboxs"][4], c["bboxs"][5], c["bboxs"][0]]                                  # right r = 2, left r = 4, right 8-bit
    items = [hi.prepare_item(frame, d) for d in dets]                                     # (the default instance: always anti-aliased)
    for it, d, k in zip(items, dets, (4, 5, 0)):
        assert set(it) == {"img", "box_center", "box_size", "img_size", "inv_trans", "do_flip", "trans"}
        assert it["img"].shape == (1, 3, P, P) and it["img"].is_cuda and it["box_center"].shape == (1, 2)
        assert it["box_size"].shape == (1, 1) and it["img_size"].shape == (1, 2) and it["inv_trans"].shape == (1, 2, 3)
        assert it["do_flip"].shape == (1,) and isinstance(it["trans"], np.ndarray) and it["trans"].shape == (2, 3)
        cx, cy, S = crop_ref.bbox_to_center_size(*d[1])
        assert it["box_center"].tolist() == [[cx, cy]] and abs(float(it["box_size"]) - S) < 1e-3 and it["img_size"].tolist() == [[640.0, 480.0]]
        assert float(it["do_flip"]) == (0.0 if d[0] == "right" else 1.0)
        np.testing.assert_allclose(it["trans"], crop_ref.gen_trans_from_patch(cx, cy, S, S, P, P), rtol=1e-12, atol=1e-9)
        dist = float(np.abs(it["img"][0].cpu().numpy().astype(np.float64) - c["truth"][k]).max())
        print(f"[crop_aa] prepare_item {d[0]} hand: |gpu - fp64| {dist:.3e} (bound {cases['bound']:.3e})")
        assert dist <= cases["bound"]
    rows = torch.cat([it["img"] for it in items])
    on = hi_aa.prepare_batch_bbox(frame, dets)
    assert torch.equal(on["img"], rows)                                                   # the switch: prepare_item's bytes
    assert torch.equal(hi.prepare_batch_frames([torch.from_numpy(frame).to(DEV)], [dets], antialias=True)["img"], rows)
    off = hi.prepare_batch_bbox(frame, dets)
    plain = ops.crop_batch(torch.from_numpy(frame).to(DEV), ops.crop_boxes(_scalars(dets), P).to(DEV), MEAN, STD, P)
    assert torch.equal(off["img"], plain) and not torch.equal(off["img"][0], rows[0]) and torch.equal(off["img"][2], rows[2])
    for k in ("box_center", "box_size", "img_size", "trans", "inv_trans", "do_flip"):
        assert torch.equal(on[k], off[k])

    # wiring: estimate_from_rgb with the switch on is _estimate over the prepare_item rows
    K = np.array([[600.0, 0, 320], [0, 610.0, 240], [0, 0, 1]], np.float32)
    out_on, _ = hi_aa.estimate_from_rgb(frame, dets, K)
    batch = {"img": rows.clone(), "box_center": torch.cat([it["box_center"] for it in items]),
             "box_size": torch.cat([it["box_size"] for it in items]).view(-1), "img_size": torch.cat([it["img_size"] for it in items]),
             "inv_trans": torch.cat([it["inv_trans"] for it in items]), "trans": torch.cat([it["inv_trans"] for it in items]),
             "do_flip": torch.cat([it["do_flip"] for it in items])}
    want, _ = hi._estimate(batch, K)
    assert torch.equal(out_on["img"], rows)
    for k in ("pred_cam_t_full", "pred_keypoints_2d_full", "pred_vertices", "pred_cam"):
        np.testing.assert_allclose(out_on[k].float().cpu().numpy(), want[k].float().cpu().numpy(), atol=1e-6, rtol=0)
    out_off, _ = hi.estimate_from_rgb(frame, dets, K)
    assert not torch.equal(out_on["pred_vertices"][:2], out_off["pred_vertices"][:2])                     # (it reaches the model)


class _FixedDetector:
    def __init__(self, dets):
        self.dets = dets

    def detect(self, image):
        return [None], [self.dets]


def test_driver_flag(hi, hi_aa, tmp_path):
    """The folder driver inherits the switch: its records are the per-frame estimate_from_rgb results of the instance it is
    handed (each forward here is one frame's two hands, the batch estimate_from_rgb runs, so the numbers are the same)."""
    from PIL import Image
    img_dir = tmp_path / "rgb"
    img_dir.mkdir()
    frames = [_noise(480, 640, 31), _noise(480, 640, 32)]
    for i, fr in enumerate(frames):
        Image.fromarray(fr[:, :, ::-1]).save(img_dir / f"f{i}.png")
    dets = [["right", [170.0, 120.0, 470.0, 360.0]], ["left", [100.0, 60.0, 540.0, 400.0]]]
    K = np.array([[600.0, 0, 320], [0, 610.0, 240], [0, 0, 1]], np.float32)
    recs = {}
    for name, h in (("on", hi_aa), ("off", hi)):
        out_dir = tmp_path / name
        st = process_batch_manopara(str(img_dir), str(out_dir), K, hamer=h, detector=_FixedDetector(dets), hands_per_forward=2)
        assert st["frames"] == 2 and st["hands"] == 4 and st["forward_sizes"] == [2, 2]
        for i, fr in enumerate(frames):
            rec = np.load(out_dir / f"f{i}.npy", allow_pickle=True).item()
            out, _ = h.estimate_from_rgb(fr, dets, K)
            for j, d in enumerate(dets):
                want = hand_record(out, d[0] == "right", j)
                for k in ("betas", "theta", "cam_t"):
                    np.testing.assert_allclose(rec[d[0]][k], want[k], atol=1e-6, rtol=0)
            recs[name, i] = rec
    for i in range(2):
        assert not np.array_equal(recs["on", i]["right"]["theta"], recs["off", i]["right"]["theta"])
