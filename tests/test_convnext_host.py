"""Host checks of the ConvNeXt-base SAR backbone (EstimateRGB(backbone='convnext')): the rule of tests/convnext_rule.py pinned
to the fixture the reference's own module wrote (tools/gen_golden_convnext.py), the key map, the load-time folding, the four
additive C entry points and their argument checks (all of which return before any launch), the public switches and the
synthetic weights.  No GPU."""
import ctypes as C
import inspect
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import convnext_rule as CR  # noqa: E402
import sar_rule as R  # noqa: E402

from hamer_yolo_amd import lib as L  # noqa: E402
from hamer_yolo_amd import synth  # noqa: E402
from hamer_yolo_amd.rootnet import convnext_arch as arch  # noqa: E402
from hamer_yolo_amd.rootnet import convnext_engine as CE  # noqa: E402
from hamer_yolo_amd.rootnet.Model_RGB import EstimateRGB  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "convnext_base.npz"))
HM_ERR_ARG = -1            # hamer_yolo_amd/csrc/common.h
NEW = ["hm_dwconv7_ln", "hm_ln_patchify2", "hm_stem4_im2col", "hm_sar_saigb_ch"]
P16, P8, P4 = C.c_void_p(16), C.c_void_p(8), C.c_void_p(4)      # fake device pointers by alignment, never dereferenced
F = C.c_float(1e-6)


@pytest.fixture(scope="module")
def sd():
    return synth.convnext_state_dict(0)


def _imgs():
    return torch.cat([CR.patches(int(s)) for s in GOLD["seeds"]])


def test_fixture_holds_data_only_and_is_small():
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "convnext_base.npz")) < 700 * 1024
    assert sorted(GOLD.files) == ["fp32_fp64_distance", "out", "seeds", "state_dict_keys", "state_dict_shapes", "tap0", "tap1", "tap2",
                                  "tap3", "tap4"]
    assert all(GOLD[k].dtype.kind in "fiU" for k in GOLD.files)          # numbers and a list of names: nothing executable
    assert GOLD["out"].shape == (2, 8, 8, 1024)
    assert 0 < float(GOLD["fp32_fp64_distance"]) < 2e-5


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_rule_matches_the_references_module(sd, dtype):
    """Bound: 4 x the distance between the reference's own fp32 and fp64 evaluations, stored in the fixture: two fp32
    evaluations of one function in different summation orders differ by about twice their distance to fp64, and the factor
    2 on top is margin.  The stream samples after the stem and each stage localise a failure."""
    bound = 4 * float(GOLD["fp32_fp64_distance"])
    out, seen = CR.forward(sd, _imgs(), dtype=dtype, taps=True)
    assert out.dtype == dtype and out.shape == (2, 8, 8, 1024)
    for i, t in enumerate(CR.tap_sample(seen)):
        ref = GOLD[f"tap{i}"]
        err = float((t.double() - torch.from_numpy(ref).double()).abs().max())
        assert err <= bound * max(1.0, float(np.abs(ref).max()) / float(np.abs(GOLD["out"]).max())), (i, err, bound)
    err = float((out.double() - torch.from_numpy(GOLD["out"]).double()).abs().max())
    print(f"rule {dtype} vs the reference's fp32 module: {err:.3e} (bound {bound:.3e})")
    assert err <= bound, (err, bound)


def test_f16_emulation_is_the_same_function_with_roundings(sd):
    """emu='f16' stays near the fp64 evaluation (the issue's CPU probe: 8.8e-4 of max |feature|; a wrong rounding point or
    a wrong fold would be far off) and the final map is f16-representable."""
    img = _imgs()[:1]
    exact = CR.forward(sd, img, dtype=torch.float64)
    emu = CR.forward(sd, img, dtype=torch.float64, emu="f16")
    assert torch.equal(emu, emu.half().double())
    rel = float((emu - exact).abs().max() / exact.abs().max())
    print(f"f16 emulation vs fp64: {rel:.3e} of max |feature| {float(exact.abs().max()):.3f}")
    assert 1e-5 < rel < 5e-3, rel


def test_key_map_covers_the_state_dict_once(sd):
    """Every non-head key of the reference module's state dict (its names and shapes are what synth reproduces and what
    tools/gen_golden_convnext.py loaded with only head.* missing) is read, none twice."""
    shapes = arch.key_shapes()
    ref = {arch.PREFIX + str(k): tuple(int(d) for d in str(s).split("x")) for k, s in zip(GOLD["state_dict_keys"], GOLD["state_dict_shapes"])}
    assert sorted(k for k in ref if k.startswith(arch.PREFIX + "head.")) == [arch.PREFIX + u for u in sorted(arch.UNUSED)]
    assert ref[arch.PREFIX + "head.weight"] == (arch.NUM_CLASSES, 1024)
    assert shapes == {k: s for k, s in ref.items() if not k.startswith(arch.PREFIX + "head.")}       # the reference module's own names
    assert set(shapes) == set(sd) and all(tuple(sd[k].shape) == s for k, s in shapes.items())
    assert not any(k.startswith(arch.PREFIX + "head.") for k in shapes)
    assert len(shapes) == 4 + 3 * 4 + 36 * 9 + 2
    assert len(arch.blocks()) == 36 and [c for _, _, c in arch.blocks()].count(512) == 27
    reads = {}

    class Counting(dict):
        def __getitem__(self, k):
            reads[k] = reads.get(k, 0) + 1
            return dict.__getitem__(self, k)

    base = CE.host_weights(Counting(sd))
    assert reads == {k: 1 for k in shapes}
    with_head = {**sd, arch.PREFIX + "head.weight": torch.zeros(4, 1024), arch.PREFIX + "head.bias": torch.zeros(4)}
    reads.clear()
    w = CE.host_weights(Counting(with_head))
    assert not any("head." in k for k in reads)
    assert set(w) == set(base) and all(torch.equal(w[n], base[n]) for n in w)
    broken = dict(sd)
    broken.pop(arch.PREFIX + "stages.2.26.pwconv2.bias")
    with pytest.raises(KeyError, match="stages.2.26.pwconv2.bias"):
        CE.host_weights(broken)


def test_folded_gamma_reproduces_the_block_in_fp64(sd):
    d = {k[len(arch.PREFIX):]: v.double() for k, v in sd.items()}
    g = torch.Generator().manual_seed(3)
    for pre, c, hw in (("stages.0.1.", 128, 12), ("stages.3.2.", 1024, 8)):
        x = torch.randn(2, hw, hw, c, generator=g, dtype=torch.float64)
        a, b = CR.block(d, pre, x), CR.block(d, pre, x, fold=True)
        assert float((a - b).abs().max()) <= 1e-12
        w = CE.host_weights(sd)
        n = [p for p, _, _ in arch.blocks()].index(arch.PREFIX + pre)
        w2, b2 = CR.folded_pwconv2({k: v.float() for k, v in d.items()}, pre)
        assert torch.equal(w[f"b{n}.w2"], w2) and torch.equal(w[f"b{n}.b2"], b2)
        assert torch.equal(w[f"b{n}.dw_w"], sd[arch.PREFIX + pre + "dwconv.weight"].reshape(c, 49).t())


def test_downsample_and_stem_weights_follow_the_kernels_k_order(sd):
    w = CE.host_weights(sd)
    stem = sd[arch.PREFIX + "downsample_layers.0.0.weight"]
    assert w["stem.w"].shape == (128, 64) and not w["stem.w"][:, 48:].any()
    assert w["stem.w"][5, 1 * 16 + 2 * 4 + 3] == stem[5, 1, 2, 3]
    dw = sd[arch.PREFIX + "downsample_layers.2.1.weight"]
    assert w["2.down.w"].shape == (512, 1024) and w["2.down.w"][7, (1 * 2 + 0) * 256 + 9] == dw[7, 9, 1, 0]
    # the 2 x 2 convolution as the patchify + GEMM computes it
    x = torch.randn(1, 4, 6, 256, dtype=torch.float64)
    ref = torch.nn.functional.conv2d(x.permute(0, 3, 1, 2), dw.double(), stride=2).permute(0, 2, 3, 1)
    rows = x.reshape(1, 2, 2, 3, 2, 256).permute(0, 1, 3, 2, 4, 5).reshape(6, 1024)
    np.testing.assert_allclose((rows @ w["2.down.w"].double().t()).reshape(1, 2, 3, 512).numpy(), ref.numpy(), atol=1e-12)


def test_exports_in_header_binding_and_library():
    hdr = open(os.path.join(ROOT, "include", "hamer_hip.h")).read()
    lib = L.load()
    for name in NEW:
        assert re.search(r"\bint " + name + r"\(", hdr), name
        assert name in L.EXPORTS, name
        assert getattr(lib, name).argtypes is not None, name
    assert int(re.search(r"#define HM_VERSION (\d+)", hdr).group(1)) == 402 == L.HM_VERSION == lib.hm_version()
    from hamer_yolo_amd import build
    assert "convnext.hip" in build.SOURCES


def test_dwconv7_ln_rejects_bad_arguments():
    lib = L.load()
    ok = dict(x=P16, w=P16, bias=P16, gamma=P16, beta=P16, out=P16, B=1, H=8, W=8, C=128, dtype=L.HM_DTYPE_F16)
    bad = [dict(x=None), dict(w=None), dict(bias=None), dict(gamma=None), dict(beta=None), dict(out=None), dict(B=0), dict(H=0),
           dict(W=-1), dict(C=0), dict(C=130), dict(C=1028), dict(C=2048), dict(x=P8), dict(w=P8), dict(out=P4),
           dict(dtype=L.HM_DTYPE_F32), dict(dtype=7), dict(B=1 << 20, H=64, W=64)]
    for kw in bad:
        a = {**ok, **kw}
        rc = lib.hm_dwconv7_ln(a["x"], a["w"], a["bias"], a["gamma"], a["beta"], a["out"], a["B"], a["H"], a["W"], a["C"], F, a["dtype"], None)
        assert rc == HM_ERR_ARG, kw
        assert b"hm_dwconv7_ln" in lib.hm_last_error_string(), kw


def test_ln_patchify2_and_stem_reject_bad_arguments():
    lib = L.load()
    ok = dict(x=P16, gamma=P16, beta=P16, out=P16, B=1, H=8, W=8, C=128, dtype=L.HM_DTYPE_F16)
    bad = [dict(x=None), dict(gamma=None), dict(beta=None), dict(out=None), dict(B=0), dict(H=7), dict(W=9), dict(H=0), dict(C=0),
           dict(C=126), dict(C=1032), dict(x=P8), dict(out=P4), dict(dtype=L.HM_DTYPE_F32)]
    for kw in bad:
        a = {**ok, **kw}
        assert lib.hm_ln_patchify2(a["x"], a["gamma"], a["beta"], a["out"], a["B"], a["H"], a["W"], a["C"], F, a["dtype"], None) == HM_ERR_ARG, kw
        assert b"hm_ln_patchify2" in lib.hm_last_error_string(), kw
    for img, out, B, H, W, dt in ((None, P16, 1, 256, 256, 1), (P16, None, 1, 256, 256, 1), (P16, P16, 0, 256, 256, 1),
                                  (P16, P16, 1, 254, 256, 1), (P16, P16, 1, 256, 250, 1), (P8, P16, 1, 256, 256, 1),
                                  (P16, P4, 1, 256, 256, 1), (P16, P16, 1, 256, 256, L.HM_DTYPE_F32)):
        assert lib.hm_stem4_im2col(img, out, B, H, W, dt, None) == HM_ERR_ARG, (img, out, B, H, W, dt)
        assert b"hm_stem4_im2col" in lib.hm_last_error_string()


def test_saigb_ch_rejects_bad_arguments():
    lib = L.load()
    ok = dict(feat=P16, w=P16, bias=P16, tmpl=P16, g=P16, B=1, ch=1024)
    for k, v in (("feat", None), ("w", None), ("bias", None), ("tmpl", None), ("g", None), ("B", 0), ("ch", 768), ("ch", 0),
                 ("ch", 2048), ("feat", P8), ("w", P8)):
        a = {**ok, k: v}
        assert lib.hm_sar_saigb_ch(a["feat"], a["w"], a["bias"], a["tmpl"], a["g"], a["B"], a["ch"], None) == HM_ERR_ARG, (k, v)
        assert b"hm_sar_saigb_ch" in lib.hm_last_error_string(), (k, v)
    assert lib.hm_sar_saigb(None, P16, P16, P16, P16, 1, None) == HM_ERR_ARG        # the old entry point keeps its own name
    assert lib.hm_last_error_string() == b"hm_sar_saigb: bad arguments"


def _cfg(**kw):
    base = dict(backbone="convnext", checkpoint="synthetic:0", device="cuda")
    return types.SimpleNamespace(**{**base, **kw})


def test_convnext_needs_in_channels_1024():
    for kw in ({}, dict(in_channels=512), dict(in_channels=768), dict(in_channels=None)):
        with pytest.raises(NotImplementedError, match="convnext") as e:
            EstimateRGB(_cfg(**kw))
        assert "1024" in str(e.value)
    with pytest.raises(NotImplementedError, match="resnet34"):
        EstimateRGB(_cfg(backbone="resnet50", in_channels=2048))


def test_precise_convnext_is_refused_before_any_device_work(monkeypatch):
    monkeypatch.setattr(synth, "convnext_state_dict", lambda *a, **k: (_ for _ in ()).throw(AssertionError("weights were built")))
    for kw, arg in ((dict(in_channels=1024), True), (dict(in_channels=1024, precise=True), None)):
        with pytest.raises(ValueError, match="fp32 route") as e:
            EstimateRGB(_cfg(**kw), precise=arg)
        assert "convnext" in str(e.value)


def test_accepted_config_reaches_the_device_check(monkeypatch):
    """backbone='convnext' with in_channels=1024 passes the configuration checks: without a GPU the next stop is the
    device check (HipLibraryError), as for the ResNet route."""
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    tiny = {}
    monkeypatch.setattr(synth, "convnext_state_dict", lambda seed=0, prefix="backbone.": tiny)
    monkeypatch.setattr(synth, "sar_head_state_dict", lambda seed=0, in_channels=512: tiny)
    with pytest.raises(L.HipLibraryError):
        EstimateRGB(_cfg(in_channels=1024))


def test_engine_constructors_and_cli():
    from hamer_yolo_amd import d_infer
    from hamer_yolo_amd.rootnet import sar_config_stage_1 as cfgmod
    from hamer_yolo_amd.rootnet.sar import SarHeadEngine
    assert inspect.signature(SarHeadEngine.__init__).parameters["in_channels"].default == 512
    with pytest.raises(ValueError):
        SarHeadEngine({}, in_channels=768)
    with pytest.raises(ValueError, match="fp32 route"):
        SarHeadEngine({}, precise=True, in_channels=1024)
    with pytest.raises(ValueError, match="fp32 route"):
        CE.ConvNextEngine({}, None, dtype=torch.float32)
    for name in ("features", "forward", "depth_of"):
        from hamer_yolo_amd.rootnet.engine import RootNetEngine
        assert list(inspect.signature(getattr(CE.ConvNextEngine, name)).parameters) == \
            list(inspect.signature(getattr(RootNetEngine, name)).parameters), name
    base = ["--input", "a", "--output", "b", "--intrinsics", "k.txt"]
    assert d_infer._parser().parse_args(base).rootnet_backbone is None
    assert cfgmod.rgb_opt.backbone == "resnet34" and cfgmod.rgb_opt.in_channels == 512
    old = cfgmod.rgb_opt.backbone, cfgmod.rgb_opt.in_channels
    try:
        d_infer.apply_rootnet_backbone(d_infer._parser().parse_args(base))
        assert (cfgmod.rgb_opt.backbone, cfgmod.rgb_opt.in_channels) == old
        d_infer.apply_rootnet_backbone(d_infer._parser().parse_args(base + ["--rootnet-backbone", "convnext"]))
        assert (cfgmod.rgb_opt.backbone, cfgmod.rgb_opt.in_channels) == ("convnext", 1024)
        d_infer.apply_rootnet_backbone(d_infer._parser().parse_args(base + ["--rootnet-backbone", "resnet34"]))
        assert (cfgmod.rgb_opt.backbone, cfgmod.rgb_opt.in_channels) == ("resnet34", 512)
    finally:
        cfgmod.rgb_opt.backbone, cfgmod.rgb_opt.in_channels = old


def test_engine_keeps_16_bit_gemm_weights_and_no_classifier(sd, monkeypatch):
    """Construction only (no launch): GEMM weights in the operand type, everything else fp32, the classifier not held."""
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    with_head = {**sd, arch.PREFIX + "head.weight": torch.zeros(arch.NUM_CLASSES, 1024), arch.PREFIX + "head.bias": torch.zeros(arch.NUM_CLASSES)}
    e = CE.ConvNextEngine(with_head, synth.convnext_rootnet_state_dict(0), device="cpu")
    assert e.dt == L.HM_DTYPE_F16 and not e.precise
    for k, v in e.w.items():
        assert v.dtype == (torch.float16 if k.endswith(("stem.w", "down.w", "w1", "w2")) else torch.float32), k
    bare = CE.ConvNextEngine(sd, None, device="cpu", dtype=torch.bfloat16)
    assert bare.dt == L.HM_DTYPE_BF16
    assert e.weight_bytes() == bare.weight_bytes() + 4 * 1024                # the depth layer; not the classifier's 45 MB
    assert e.weight_bytes() <= 2 * sum(v.numel() for v in sd.values()) + (4 << 20)      # fp32 vectors and depthwise taps on top
    with pytest.raises(ValueError, match="1024"):
        CE.ConvNextEngine(sd, synth.rootnet_state_dict(0)[1], device="cpu")


def test_sar_head_state_dict_default_is_unchanged():
    a, b = synth.sar_head_state_dict(0), synth.sar_head_state_dict(0, in_channels=512)
    assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)
    gold = np.load(os.path.join(ROOT, "tests", "golden", "sar_head.npz"))
    np.testing.assert_allclose(R.head(a, torch.from_numpy(gold["feats"]).float()).numpy(), gold["coords"], rtol=0, atol=1e-6)
    c = synth.sar_head_state_dict(0, in_channels=1024)
    assert c["head.saigb.group.0.weight"].shape == (6224, 1024, 1, 1)
    assert all(torch.equal(a[k], c[k]) for k in a if k != "head.saigb.group.0.weight")


def test_synthetic_layer_scale_and_peaked_heatmaps(sd):
    """The calibration the parity tests rest on: layer scale of order 0.1 .. 1 (the blocks matter), and the 1024-channel
    head on this backbone's features sees peaked, spread-out heatmaps (DESIGN section 9 records what near-tied ones do)."""
    for pre, _, _ in arch.blocks():
        g = sd[pre + "gamma"]
        assert 0.09 <= float(g.min()) and float(g.max()) <= 0.51
    feat = torch.from_numpy(GOLD["out"]).permute(0, 3, 1, 2).contiguous()
    assert abs(float(feat.std()) - 1.0) < 0.15 and abs(float(feat.mean())) < 0.1
    coords, p = R.head(synth.sar_head_state_dict(0, in_channels=1024), feat, return_heatmaps=True)
    assert float(p.flatten(2).max(2)[0].mean()) >= 0.05
    cells = (coords[:, :, :2] + 1) * 16
    assert float(cells[:, :, 0].max() - cells[:, :, 0].min()) >= 8 and float(cells[:, :, 1].max() - cells[:, :, 1].min()) >= 8
