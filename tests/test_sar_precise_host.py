"""Host checks of the precise (fp32) route of the RootNet backbone, the depth head and the SAR head: the public switches, the
CLI flag, the six additive C entry points and their argument checks (all of which return before any launch), the fp32
weights the engines keep, and the fp64 oracle of tests/sar_precise_chain.py pinned to the fp32 rule.  No GPU."""
import ctypes as C
import inspect
import os
import re
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sar_precise_chain as PC  # noqa: E402
import sar_rule as R  # noqa: E402

from hamer_yolo_amd import lib as L  # noqa: E402
from hamer_yolo_amd import synth  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HM_ERR_ARG = -1            # hamer_yolo_amd/csrc/common.h
NEW = ["hm_conv2d_f32_relu", "hm_nchw3_to_nhwc8_f32", "hm_gap_linear_f32", "hm_sar_saigb_f32", "hm_sar_graph_mix_f32",
       "hm_sar_linear_f32"]
P16, P8 = C.c_void_p(16), C.c_void_p(8)      # fake device pointers: 16-byte aligned / only 8-byte aligned, never dereferenced


def test_config_default_and_cli_flag():
    from hamer_yolo_amd import d_infer
    from hamer_yolo_amd.rootnet.sar_config_stage_1 import rgb_opt
    assert rgb_opt.precise is False
    base = ["--input", "a", "--output", "b", "--intrinsics", "k.txt"]
    assert d_infer._parser().parse_args(base).precise_rootnet is False
    args = d_infer._parser().parse_args(base + ["--precise-rootnet", "--precise-detector"])
    assert args.precise_rootnet is True and args.precise_detector is True


def test_constructors_take_the_new_arguments():
    from hamer_yolo_amd.rootnet.engine import RootNetEngine
    from hamer_yolo_amd.rootnet.Model_RGB import EstimateRGB
    from hamer_yolo_amd.rootnet.sar import SarHeadEngine
    assert inspect.signature(EstimateRGB.__init__).parameters["precise"].default is None
    assert inspect.signature(SarHeadEngine.__init__).parameters["precise"].default is False
    assert inspect.signature(RootNetEngine.__init__).parameters["dtype"].default is torch.float16


def test_engines_keep_fp32_operands_on_the_precise_route(monkeypatch):
    """Construction only (no launch): an fp32 request maps to HM_DTYPE_F32, never to fp16, and the weights stay fp32."""
    from hamer_yolo_amd.rootnet.engine import RootNetEngine
    from hamer_yolo_amd.rootnet.sar import SarHeadEngine
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    net, root = synth.rootnet_state_dict(0)
    e32 = RootNetEngine(net, root, device="cpu", dtype=torch.float32)
    assert e32.precise and e32.dt == L.HM_DTYPE_F32
    assert all(w.dtype == torch.float32 for w, *_ in e32.w.values())
    e16 = RootNetEngine(net, root, device="cpu")
    assert not e16.precise and e16.dt == L.HM_DTYPE_F16 and e16.w["stem"][0].dtype == torch.float16
    assert RootNetEngine(net, root, device="cpu", dtype=torch.bfloat16).dt == L.HM_DTYPE_BF16
    sd = synth.sar_head_state_dict(0)
    h32 = SarHeadEngine(sd, device="cpu", precise=True)
    assert h32.precise and all(v.dtype == torch.float32 for v in h32.w.values())
    ws = h32._workspace(2)
    assert all(ws[k].dtype == torch.float32 for k in ("g", "mix", "h", "xy", "z"))
    h16 = SarHeadEngine(sd, device="cpu")
    assert not h16.precise and h16.w["xy.lap0"].dtype == torch.float16 and h16._workspace(2)["g"].dtype == torch.float16


def test_exports_in_header_and_binding():
    hdr = open(os.path.join(ROOT, "include", "hamer_hip.h")).read()
    lib = L.load()
    for name in NEW:
        assert re.search(r"\bint " + name + r"\(", hdr), name
        assert name in L.EXPORTS, name
        assert getattr(lib, name).argtypes is not None, name
    assert int(re.search(r"#define HM_VERSION (\d+)", hdr).group(1)) == 402 == L.HM_VERSION == lib.hm_version()


def _conv(**kw):
    """ResNet-34 layer-3 conv, 3x3 s1 on 16x16, 256 -> 256, fp32, ReLU.  Fake, never dereferenced pointers."""
    a = L.ConvArgs(16, 16, 16, 16, 16, 4, 16, 16, 256, 256, 3, 1, 256, 256, 2304, 2, 0, L.HM_DTYPE_F32)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_conv2d_f32_relu_rejects_bad_arguments():
    lib = L.load()
    bad = [dict(dtype=L.HM_DTYPE_F16), dict(dtype=L.HM_DTYPE_BF16), dict(act=1), dict(act=3), dict(out_f32=1), dict(X=0),
           dict(W=0), dict(Y=0), dict(bias=0), dict(N=0), dict(Cout=0), dict(ksize=5 + 1), dict(stride=3), dict(Cin=24, ldx=24),
           dict(Kpad=2300), dict(Kpad=1024), dict(X=8), dict(W=8), dict(Y=2), dict(ldx=254), dict(resid=16, ldr=128),
           dict(resid=2, ldr=256)]
    for kw in bad:
        assert lib.hm_conv2d_f32_relu(C.byref(_conv(**kw)), None) == HM_ERR_ARG, kw
        assert b"hm_conv2d_f32_relu" in lib.hm_last_error_string(), kw
    assert lib.hm_conv2d_f32_relu(None, None) == HM_ERR_ARG


def test_fp32_root_ops_reject_bad_arguments():
    lib = L.load()
    assert lib.hm_nchw3_to_nhwc8_f32(None, P16, 1, 8, 8, None) == HM_ERR_ARG
    assert lib.hm_nchw3_to_nhwc8_f32(P16, None, 1, 8, 8, None) == HM_ERR_ARG
    assert lib.hm_nchw3_to_nhwc8_f32(P16, P8, 1, 8, 8, None) == HM_ERR_ARG
    for B, H, W in ((0, 8, 8), (1, 0, 8), (1, 8, 0)):
        assert lib.hm_nchw3_to_nhwc8_f32(P16, P16, B, H, W, None) == HM_ERR_ARG
    f0 = C.c_float(0.0)
    assert lib.hm_gap_linear_f32(None, 64, 512, P16, f0, P16, P16, 1, None) == HM_ERR_ARG
    assert lib.hm_gap_linear_f32(P16, 64, 512, P16, f0, None, P16, 1, None) == HM_ERR_ARG
    assert lib.hm_gap_linear_f32(C.c_void_p(18), 64, 512, P16, f0, P16, P16, 1, None) == HM_ERR_ARG
    for hw, c, b in ((0, 512, 1), (64, 0, 1), (64, 512, 0)):
        assert lib.hm_gap_linear_f32(P16, hw, c, P16, f0, P16, P16, b, None) == HM_ERR_ARG
    assert b"hm_gap_linear_f32" in lib.hm_last_error_string()


def test_fp32_head_gemms_reject_bad_arguments():
    lib = L.load()
    ok = dict(feat=P16, w=P16, bias=P16, tmpl=P16, g=P16, B=1)
    for k, v in (("feat", None), ("w", None), ("bias", None), ("tmpl", None), ("g", None), ("B", 0), ("feat", P8), ("w", P8)):
        a = {**ok, k: v}
        assert lib.hm_sar_saigb_f32(a["feat"], a["w"], a["bias"], a["tmpl"], a["g"], a["B"], None) == HM_ERR_ARG, k
    assert b"hm_sar_saigb_f32" in lib.hm_last_error_string()
    for lap, ldl, x, N, y in ((None, 800, P16, 544, P16), (P16, 800, None, 544, P16), (P16, 800, P16, 544, None),
                              (P16, 776, P16, 544, P16), (P16, 802, P16, 544, P16), (P16, 800, P16, 0, P16),
                              (P16, 800, P16, 546, P16), (P8, 800, P16, 544, P16), (P16, 800, P8, 544, P16)):
        assert lib.hm_sar_graph_mix_f32(lap, ldl, x, N, y, None) == HM_ERR_ARG, (lap, ldl, x, N, y)
    assert b"hm_sar_graph_mix_f32" in lib.hm_last_error_string()
    for x, M, K, w, N, lg in ((None, 778, 544, P16, 1024, 0), (P16, 778, 544, None, 1024, 0), (P16, 0, 544, P16, 1024, 0),
                              (P16, 778, 0, P16, 1024, 0), (P16, 778, 515, P16, 1024, 0), (P16, 778, 544, P16, 0, 0),
                              (P16, 778, 544, P16, 1024, 2), (P8, 778, 544, P16, 1024, 1), (P16, 778, 544, P8, 1024, 1)):
        assert lib.hm_sar_linear_f32(x, M, K, w, P16, P16, N, lg, None) == HM_ERR_ARG, (x, M, K, w, N, lg)
    assert lib.hm_sar_linear_f32(P16, 778, 544, P16, None, P16, 1024, 0, None) == HM_ERR_ARG
    assert lib.hm_sar_linear_f32(P16, 778, 544, P16, P16, None, 1024, 0, None) == HM_ERR_ARG
    assert b"hm_sar_linear_f32" in lib.hm_last_error_string()


def test_fp32_refusals_of_the_default_entry_points_stay():
    """The additive route leaves the old refusals as they were (tests/test_host_logic_f32.py pins them too)."""
    lib = L.load()
    relu = _conv(act=2)
    assert lib.hm_conv2d_nhwc(C.byref(relu), None) == HM_ERR_ARG
    assert lib.hm_nchw3_to_nhwc8(P16, P16, 1, 8, 8, L.HM_DTYPE_F32, None) == HM_ERR_ARG


def test_fp64_chain_head_matches_fp32_rule_on_fixture():
    """The fp64 head of sar_precise_chain agrees with sar_rule.head (pinned to the reference's modules within 1e-6) within
    fp32 rounding on the committed fixture: measured 2.0e-6."""
    gold = np.load(os.path.join(ROOT, "tests", "golden", "sar_head.npz"))
    sd = synth.sar_head_state_dict(0)
    feats = torch.from_numpy(gold["feats"])
    got = PC.head(sd, feats)
    assert got.dtype == torch.float64
    err = (got - R.head(sd, feats.float()).double()).abs().amax().item()
    assert err <= 4e-6, err
    assert np.abs(got.numpy() - gold["coords"]).max() <= 4e-6
