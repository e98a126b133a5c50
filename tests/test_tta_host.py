"""Host side of the detector's test-time augmentation: the numpy rule (tests/tta_rule.py) against torch's CPU
F.interpolate + F.pad; the sizes and row counts; the library's host size / table entries against the rule, on integers and
fp32 bits; the surface (header, binding, build list, HM_VERSION); every argument refusal, without a device; the switches."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import tta_rule as TR
from hamer_yolo_amd import build as B
from hamer_yolo_amd import lib as L
from hamer_yolo_amd import ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = ((64, 96), (192, 320), (384, 640))
RATIOS = (0.83, 0.67, 0.5)


@pytest.mark.parametrize("hw", SIZES)
@pytest.mark.parametrize("ratio", RATIOS)
def test_rule_equals_torch_scale_img(hw, ratio):
    """Outputs are convex combinations of inputs in [0, 1]: about four fp32 roundings, so 1e-6 absolute."""
    g = torch.Generator().manual_seed(hw[0] * 7 + int(ratio * 100))
    x = torch.rand(2, 3, hw[0], hw[1], generator=g)
    for flip in (False, True):
        want = TR.torch_scale_img(x.flip(3) if flip else x, ratio).numpy()
        got = TR.scale_img(x.numpy(), ratio, flip=flip)
        assert got.shape == want.shape
        assert float(np.abs(got - want.astype(np.float64)).max()) <= 1e-6
        sh, sw, hp, wp = TR.sizes(hw[0], hw[1], ratio)
        assert np.all(got[..., sh:, :] == 0.447) and np.all(got[..., :, sw:] == 0.447)


def test_sizes_and_row_counts():
    assert TR.sizes(384, 640, 0.83) == (318, 531, 320, 544) and TR.sizes(384, 640, 0.67) == (257, 428, 288, 448)
    assert TR.sizes(192, 320, 0.83) == (159, 265, 160, 288) and TR.sizes(192, 320, 0.67) == (128, 214, 160, 224)
    assert TR.sizes(128, 192, 0.5) == (64, 96, 64, 96) and TR.sizes(384, 640, 1.0) == (384, 640, 384, 640)
    assert TR.n_rows(384, 640) == ([15120, 10710, 7938], 33768)
    assert TR.n_rows(192, 320) == ([3780, 2835, 2205], 8820)
    assert (245760 + 174080 + 129024) / 245760 == pytest.approx(2.233, abs=1e-3)       # the input-area ratio of a 1080p pass
    assert TR.SCALES == (1.0, 0.83, 0.67) and TR.FLIPS == (False, True, False)


def test_descale_and_deflip():
    p = np.array([[100.0, 50.0, 20.0, 10.0, 0.5, 0.25, 0.75, 0.1]], np.float32)
    d = TR.descale(p, 0.83, True, 640)
    assert d.dtype == np.float32
    assert np.array_equal(d[0, 1:4], p[0, 1:4] / np.float32(0.83)) and d[0, 0] == np.float32(640) - p[0, 0] / np.float32(0.83)
    assert np.array_equal(d[0, 4:], p[0, 4:])
    t = torch.from_numpy(p.copy())
    t[..., :4] /= 0.83
    t[..., 0] = 640 - t[..., 0]
    assert np.array_equal(t.numpy().view(np.uint32), d.view(np.uint32))                 # torch's CPU arithmetic, bit for bit
    assert np.array_equal(TR.descale(p, 1.0, False, 640), p)


@pytest.mark.parametrize("hw", SIZES + ((128, 192), (640, 640)))
@pytest.mark.parametrize("ratio", RATIOS + (1.0,))
def test_library_sizes_and_tables_equal_the_rule(hw, ratio):
    assert ops.tta_sizes(hw[0], hw[1], ratio, 32) == TR.sizes(hw[0], hw[1], ratio)
    for flip in (False, True):
        got = ops.tta_tables(hw[0], hw[1], ratio, 32, flip).numpy()
        want = TR.table(hw[0], hw[1], ratio, 32, flip)
        assert got.dtype == np.int32 and got.shape == want.shape and np.array_equal(got, want), (hw, ratio, flip)
    sh, sw, hp, wp = TR.sizes(hw[0], hw[1], ratio)
    t = ops.tta_tables(hw[0], hw[1], ratio, 32, True).numpy()
    assert np.all(t[sw:wp] == -1) and np.all(t[4 * wp + sh:4 * wp + hp] == -1)          # the padding columns and rows
    assert t[:sw].min() >= 0 and t[:sw].max() <= hw[1] - 1 and t[wp:wp + sw].min() >= 0 and t[wp:wp + sw].max() <= hw[1] - 1
    w0, w1 = t[2 * wp:2 * wp + sw].view(np.float32), t[3 * wp:3 * wp + sw].view(np.float32)
    assert np.all((w0 >= 0) & (w0 <= 1) & (w1 >= 0) & (w1 <= 1))


def test_taps_are_torchs_own():
    """A one-hot row through torch's resize shows torch's taps: the rule's table names the same two pixels."""
    for sn, ratio in ((96, 0.83), (320, 0.67), (640, 0.83)):
        dn = int(sn * ratio)
        i0, i1, l0, l1 = TR.taps(sn, dn, dn)
        eye = torch.eye(sn).reshape(1, sn, 1, sn)                                       # channel j: the one-hot of pixel j
        out = F.interpolate(eye.expand(1, sn, 2, sn), size=(2, dn), mode='bilinear', align_corners=False)[0, :, 0]   # (sn, dn)
        for d in range(dn):
            nz = set(torch.nonzero(out[:, d]).flatten().tolist())
            mine = {int(i) for i, l in ((i0[d], l0[d]), (i1[d], l1[d])) if l != 0}
            assert nz == mine, (sn, ratio, d, nz, mine)


NEW = ("hm_tta_sizes", "hm_tta_tables", "hm_tta_scale", "hm_yolo_decode_batch_tta")


def test_surface():
    header = open(os.path.join(ROOT, "include", "hamer_hip.h")).read()
    lib = L.load()
    for name in NEW:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in L.EXPORTS and hasattr(lib, name), name
    for word in ("0.83", "0.67", "0.447", "align_corners=False", "yolo.py:589-605"):
        assert word in header, word                                                     # the rule is in the comment
    assert "tta.hip" in B.SOURCES and os.path.exists(os.path.join(B.CSRC, "tta.hip"))
    assert re.search(r"#define HM_VERSION 402\b", header) and L.HM_VERSION == 402 and lib.hm_version() == 402
    for name in ("tta_sizes", "tta_tables", "tta_scale", "yolo_decode_batch_tta"):
        assert callable(getattr(ops, name))


def _buf(n=4096, align=32):
    return C.addressof(C.create_string_buffer(n + 64)) + (align - 1) & ~(align - 1)     # a non-null aligned address; errors return before device work


def _scale(**kw):
    a = dict(x=_buf(), y=_buf(), tab=_buf(), nb=1, h=64, w=96, ratio=0.83, gs=32, dtype=L.HM_DTYPE_F16)
    a.update(kw)
    return L.load().hm_tta_scale(a["x"], a["y"], a["tab"], a["nb"], a["h"], a["w"], a["ratio"], a["gs"], a["dtype"], None)


BAD_SCALE = {"x=None": dict(x=None), "y=None": dict(y=None), "tab=None": dict(tab=None), "nb=0": dict(nb=0), "nb=65536": dict(nb=65536),
             "h=0": dict(h=0), "w=-1": dict(w=-1), "gs=0": dict(gs=0), "h=16385": dict(h=16385), "ratio=0": dict(ratio=0.0),
             "ratio=-0.5": dict(ratio=-0.5), "ratio=1.01": dict(ratio=1.01), "ratio=nan": dict(ratio=float("nan")),
             "resized-to-nothing": dict(h=4, ratio=0.2), "dtype=3": dict(dtype=3), "x-misaligned": dict(x=_buf() + 8),
             "y-misaligned": dict(y=_buf() + 8), "y-16-in-fp32": dict(y=_buf() + 16, dtype=L.HM_DTYPE_F32),
             "tab-misaligned": dict(tab=_buf() + 2)}


@pytest.mark.parametrize("kw", list(BAD_SCALE.values()), ids=list(BAD_SCALE))
def test_scale_refusals_without_a_device(kw):
    rc = _scale(**kw)
    msg = L.load().hm_last_error_string().decode()
    assert rc != 0 and "hm_tta_scale" in msg, (rc, msg)


def _decode(**kw):
    a = dict(raw=_buf(), ldraw=24, pred=_buf(), row0=0, ny=2, nx=2, nc=3, stride=8.0, anc=(C.c_float * 6)(1, 2, 3, 4, 5, 6), nb=1,
             rows=12, scale=0.83, flip=1, full_w=640.0)
    a.update(kw)
    return L.load().hm_yolo_decode_batch_tta(a["raw"], a["ldraw"], a["pred"], a["row0"], a["ny"], a["nx"], a["nc"], a["stride"], a["anc"],
                                             a["nb"], a["rows"], a["scale"], a["flip"], a["full_w"], None)


BAD_DECODE = {"raw=None": dict(raw=None), "pred=None": dict(pred=None), "anchors=None": dict(anc=None), "ny=0": dict(ny=0),
              "nx=0": dict(nx=0), "nc=0": dict(nc=0), "row0=-1": dict(row0=-1), "nb=0": dict(nb=0), "nb=65536": dict(nb=65536),
              "ldraw=23": dict(ldraw=23), "scale=0": dict(scale=0.0), "scale=1.5": dict(scale=1.5), "scale=nan": dict(scale=float("nan")),
              "flip-without-width": dict(full_w=0.0)}


@pytest.mark.parametrize("kw", list(BAD_DECODE.values()), ids=list(BAD_DECODE))
def test_decode_refusals_without_a_device(kw):
    rc = _decode(**kw)
    msg = L.load().hm_last_error_string().decode()
    assert rc != 0 and "hm_yolo_decode_batch_tta" in msg, (rc, msg)


def test_host_entry_refusals():
    lib = L.load()
    sz = (C.c_int * 4)()
    tab = (C.c_int32 * 4096)()
    for args in ((0, 96, 0.83, 32), (64, 0, 0.83, 32), (64, 96, 0.0, 32), (64, 96, 1.5, 32), (64, 96, float("nan"), 32), (64, 96, 0.83, 0),
                 (64, 96, 0.01, 32)):
        assert lib.hm_tta_sizes(*args, sz) != 0 and "hm_tta_sizes" in lib.hm_last_error_string().decode(), args
        assert lib.hm_tta_tables(*args, 0, tab) != 0 and "hm_tta_tables" in lib.hm_last_error_string().decode(), args
    assert lib.hm_tta_sizes(64, 96, 0.83, 32, None) != 0 and lib.hm_tta_tables(64, 96, 0.83, 32, 0, None) != 0
    with pytest.raises(L.HipLibraryError):
        ops.tta_sizes(64, 96, 2.0)


def test_switches():
    from hamer_yolo_amd import d_infer, evaluate_det, infer
    from hamer_yolo_amd.config.yolo_config import Config, yolo_opt
    assert yolo_opt.tta is False and Config.tta is False and yolo_opt.augment is True      # augment stays the ignored field
    a = infer._parser().parse_args(["--input", "i", "--output", "o", "--tta-detector"])
    assert a.tta_detector is True and infer._parser().parse_args(["--input", "i", "--output", "o"]).tta_detector is False
    d = d_infer._parser().parse_args(["--input", "i", "--output", "o", "--intrinsics", "k", "--tta-detector"])
    assert d.tta_detector is True
    assert d_infer._parser().parse_args(["--input", "i", "--output", "o", "--intrinsics", "k"]).tta_detector is False
    for protocol in ("deployed", "test"):
        e = evaluate_det._parser().parse_args(["--labels", "l", "--images", "i", "--protocol", protocol, "--augment"])
        assert e.augment is True and e.protocol == protocol
    assert evaluate_det._parser().parse_args(["--labels", "l", "--images", "i"]).augment is False
    try:                                                                                # the flag sets the config switch, nothing else
        infer.apply_tta_args(infer._parser().parse_args(["--input", "i", "--output", "o"]))
        assert yolo_opt.tta is False
        infer.apply_tta_args(a)
        assert yolo_opt.tta is True
    finally:
        yolo_opt.__dict__.pop("tta", None)
    assert yolo_opt.tta is False


def test_detector_and_engine_signatures():
    import inspect
    from hamer_yolo_amd.yolo.detector import Detector
    from hamer_yolo_amd.yolo.engine import YoloEngine
    assert list(inspect.signature(Detector.__init__).parameters) == ["self", "config", "precise", "tta"]
    assert inspect.signature(Detector.__init__).parameters["tta"].default is None
    f = inspect.signature(YoloEngine.forward).parameters
    assert list(f) == ["self", "frame", "want_u8", "tta"] and f["tta"].default is False
    p = inspect.signature(YoloEngine._plan).parameters
    assert list(p) == ["self", "H", "W", "nb", "tta"] and p["tta"].default is False
    assert YoloEngine.TTA_SCALES == TR.SCALES and YoloEngine.TTA_FLIPS == TR.FLIPS
