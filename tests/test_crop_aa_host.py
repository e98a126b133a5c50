"""Host checks of the anti-aliased HaMeR crop (hm_crop_batch_aa, hamer_inference.prepare_item, --antialias-crop): the size rule's
known answers, the host helper hm_crop_aa_box_from_bbox against them and against hm_crop_box_from_bbox, the numpy rule of
tests/crop_aa_rule.py against scipy (the oracle of the blur) and against oracle.crop_ref where nothing is blurred, and the
surface -- exports, header, build list, keyword, command-line flag.  No GPU."""
import ctypes as C
import inspect
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import crop_aa_rule as R  # noqa: E402

from hamer_yolo_amd import build as B  # noqa: E402
from hamer_yolo_amd import lib as L  # noqa: E402
from oracle import crop_ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEAN = 255.0 * np.array([0.485, 0.456, 0.406])
STD = 255.0 * np.array([0.229, 0.224, 0.225])
# S -> (sigma, radius) at P = 256; None: the 8-bit path
KNOWN = [(563, None), (564, (0.05078125, 0)), (600, (0.0859375, 0)), (667, (0.1513671875, 1)), (1000, (0.4765625, 2)),
         (3000, (2.4296875, 10)), (6400, (5.75, 23)), (12800, (12.0, 48))]


def _helper(cx, cy, S, flip=0, P=256):
    box, taps = L.CropAaBox(), (C.c_float * L.HM_CROP_AA_TAPS)()
    rc = L.load().hm_crop_aa_box_from_bbox(float(cx), float(cy), float(S), flip, P, C.byref(box), taps)
    return rc, box, np.array(taps[:], dtype=np.float32)


@pytest.mark.parametrize("S,want", KNOWN)
def test_size_rule_known_answers(S, want):
    assert R.blur_of_size(float(S), 256) == want


@pytest.mark.parametrize("S,want", KNOWN)
def test_helper_matches_the_rule(S, want):
    rc, box, taps = _helper(317.25, 201.5, S, flip=1)
    assert rc == 0
    plain = L.CropBox()
    assert L.load().hm_crop_box_from_bbox(317.25, 201.5, float(S), 1, 256, C.byref(plain)) == 0
    for f in ("m0", "m4", "x0", "y0", "flip", "reserved"):
        assert getattr(box, f) == getattr(plain, f), f
    if want is None:
        assert box.sigma == 0.0 and box.radius == 0
        assert taps[0] == 1.0 and not taps[1:].any()
        return
    sigma, radius = want
    assert box.sigma == np.float32(sigma) and box.radius == radius
    g = R.gaussian_taps(sigma, radius)
    assert abs(g.sum() - 1.0) < 1e-15 and np.array_equal(g, g[::-1])
    assert np.array_equal(taps[:radius + 1], g[radius:].astype(np.float32))          # the double taps, rounded to fp32
    assert not taps[radius + 1:].any()


def test_helper_rejects_a_size_beyond_the_cap():
    rc, _, _ = _helper(100.0, 100.0, 12900.0)
    assert rc != 0
    msg = L.load().hm_last_error_string().decode()
    assert "12900" in msg and "hm_crop_aa_box_from_bbox" in msg
    # the radius itself: nothing above 48 passes (radius 49 begins at sigma 12.125, size 12928)
    for S in (12928.0, 20000.0, 1e9):
        assert _helper(0.0, 0.0, S)[0] != 0
    assert _helper(0.0, 0.0, 12800.0)[0] == 0
    assert L.load().hm_crop_aa_box_from_bbox(0.0, 0.0, 700.0, 0, 256, None, None) != 0


def test_rule_blur_is_scipys():
    """scipy.ndimage.gaussian_filter is what skimage.filters.gaussian runs; the rule's blur is that filter."""
    from scipy.ndimage import gaussian_filter
    img = np.random.default_rng(5).integers(0, 256, (37, 53, 3), dtype=np.uint8)
    for sigma in (0.05078125, 0.1513671875, 0.4765625, 2.4296875, 5.75):
        radius = int(4.0 * sigma + 0.5)
        want = gaussian_filter(img.astype(np.float64), (sigma, sigma, 0), mode="nearest", truncate=4.0)
        got = R.gaussian_blur(img, sigma, radius)
        assert np.abs(got - want).max() < 1e-11, sigma            # (sums of <= 47 products of values <= 255 in double)
        rows, cols = np.array([0, 3, 36]), np.array([1, 2, 52])
        assert np.array_equal(R.gaussian_blur_at(img, sigma, radius, rows, cols), got[rows][:, cols])


def test_rule_without_blur_is_the_batched_crop():
    frame = np.random.default_rng(6).integers(0, 256, (120, 160, 3), dtype=np.uint8)
    for bbox in (["right", [40.0, 30.0, 100.0, 90.0]], ["left", [-20.0, 50.0, 80.0, 130.0]], ["left", [10.0, 5.0, 150.0, 170.0]]):
        S = crop_ref.bbox_to_center_size(*bbox[1])[2]
        assert (S / 256) / 2.0 <= 1.1 and not R.is_blurred(bbox)
        want = crop_ref.prepare_batch_bbox(frame, [bbox], MEAN, STD)["img"][0]
        for dt in (np.float64, np.float32):
            assert np.array_equal(R.prepare_item_img(frame, bbox, MEAN, STD, dtype=dt), want.astype(dt))


def test_rule_keeps_a_constant_frame_constant():
    """Taps that sum to 1 and bilinear weights that sum to 1: wherever the four taps and their blur support lie inside the
    frame, a constant frame gives the constant; where taps fall outside, less."""
    H, W, v = 300, 400, 201
    frame = np.full((H, W, 3), v, dtype=np.uint8)
    for bbox in (["right", [100.0, 60.0, 300.0, 240.0]], ["left", [-50.0, -20.0, 350.0, 280.0]]):
        cx, cy, S = crop_ref.bbox_to_center_size(*bbox[1])
        sigma, radius = R.blur_of_size(S)
        assert radius >= 1
        out = R.prepare_item_img(frame, bbox, MEAN, STD)
        inside = R.interior_mask(crop_ref.gen_trans_from_patch(cx, cy, S, S, 256, 256), 256, 256, H, W, radius)
        if bbox[0] != "right":
            inside = inside[:, ::-1]
        assert inside.any() and not inside.all()
        for c in range(3):
            want = (v - float(np.float32(MEAN[c]))) / float(np.float32(STD[c]))
            assert np.abs(out[c][inside] - want).max() < 1e-12
        assert (out[0][~inside] <= (v - float(np.float32(MEAN[0]))) / float(np.float32(STD[0])) + 1e-12).all()


def test_surface():
    header = open(os.path.join(ROOT, "include", "hamer_hip.h")).read()
    lib = L.load()
    for name in ("hm_crop_aa_box_from_bbox", "hm_crop_batch_aa"):
        assert re.search(r"\bint %s\(" % name, header) and name in L.EXPORTS and hasattr(lib, name)
    assert "typedef struct hm_crop_aa_box" in header
    assert re.search(r"#define HM_VERSION 402\b", header)
    assert L.HM_VERSION == 402 and lib.hm_version() == 402
    assert "crop_aa.hip" in B.SOURCES and os.path.exists(os.path.join(B.CSRC, "crop_aa.hip"))
    assert C.sizeof(L.CropAaBox) == 48 and L.CropAaBox._fields_[:len(L.CropBox._fields_)] == L.CropBox._fields_
    assert C.sizeof(L.CropBox) == 32                                                     # hm_crop_box keeps its layout
    assert lib.hm_crop_batch_aa(None, 480, 640, None, None, None, 1, 256, None, None, None) != 0
    assert "hm_crop_batch_aa" in lib.hm_last_error_string().decode()


def test_keyword_flag_and_prepare_item_errors():
    from hamer_yolo_amd import d_infer, infer
    from hamer_yolo_amd.config.hamer_config import hamer_opt
    sig = inspect.signature(infer.hamer_inference.__init__)
    assert sig.parameters["antialias"].default is None and sig.parameters["precise"].default is None
    assert list(inspect.signature(infer.hamer_inference.prepare_item).parameters) == ["self", "img_0", "bbox"]
    base = ["--input", "i", "--output", "o"]
    for mod, extra in ((infer, []), (d_infer, ["--intrinsics", "k"])):
        assert mod._parser().parse_args(base + extra).antialias_crop is False
        assert mod._parser().parse_args(base + extra + ["--antialias-crop"]).antialias_crop is True
    from hamer_yolo_amd.config.yolo_config import yolo_opt
    saved, saved_yolo = dict(vars(hamer_opt)), dict(vars(yolo_opt))
    try:
        hamer_opt.__dict__.pop("antialias", None)
        infer.apply_antialias_args(infer._parser().parse_args(base))
        assert hamer_opt.antialias is False
        infer.apply_precise_args(infer._parser().parse_args(base + ["--precise"]))
        infer.apply_antialias_args(infer._parser().parse_args(base + ["--precise"]))
        assert hamer_opt.precise is True and hamer_opt.antialias is False        # a precision switch does not imply it
        infer.apply_antialias_args(d_infer._parser().parse_args(base + ["--intrinsics", "k", "--antialias-crop"]))
        assert hamer_opt.antialias is True
    finally:
        for opt, old in ((hamer_opt, saved), (yolo_opt, saved_yolo)):
            vars(opt).clear()
            vars(opt).update(old)
    # the two malformed shapes are refused before the frame is touched (no device, no model: self is never used)
    with pytest.raises(ValueError, match="Invalid bbox format"):
        infer.hamer_inference.prepare_item(None, None, ["right", [1.0, 2.0, 3.0, 4.0], 0])
    with pytest.raises(ValueError, match="Invalid bbox format"):
        infer.hamer_inference.prepare_item(None, None, ("right", [1.0, 2.0, 3.0, 4.0]))
    with pytest.raises(ValueError, match="Invalid coordinates format"):
        infer.hamer_inference.prepare_item(None, None, ["right", [1.0, 2.0, 3.0]])
