"""Host checks of the precise (fp32) HaMeR route: the additive C entry points and their argument checks (all return before
any launch), the emitted gfx950 code of the two new kernels, the public switches and CLI flags, HamerEngine's argument checks
(raised before any device work) and the fp64 chain of tests/hamer_precise_chain.py pinned to the fp32 oracle.  No GPU."""
import ctypes as C
import inspect
import os
import re
import subprocess
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hamer_precise_chain as PC  # noqa: E402

from hamer_yolo_amd import lib as L  # noqa: E402
from hamer_yolo_amd import synth  # noqa: E402
from oracle import hamer_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hamer_yolo_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
HM_ERR_ARG = -1
NEW = ["hm_gemm_f32", "hm_vit_attention_f32"]
P16, P8 = C.c_void_p(4096), C.c_void_p(8)      # fake device pointers, never dereferenced


def test_exports_in_header_binding_and_build_list():
    from hamer_yolo_amd import build
    hdr = open(os.path.join(ROOT, "include", "hamer_hip.h")).read()
    lib = L.load()
    for name in NEW:
        assert re.search(r"\bint " + name + r"\(", hdr), name
        assert name in L.EXPORTS, name
        assert getattr(lib, name).argtypes is not None, name
    assert int(re.search(r"#define HM_VERSION (\d+)", hdr).group(1)) == 402 == L.HM_VERSION == lib.hm_version()
    assert "gemm_f32.hip" in build.SOURCES and "attention_f32.hip" in build.SOURCES
    assert L.HM_DTYPE_F32 == int(re.search(r"HM_DTYPE_F32 = (\d+)", hdr).group(1)) == 2


def _isa(tmp_path, name):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    out = str(tmp_path / (name + ".s"))
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-S", "--cuda-device-only",
                    os.path.join(CSRC, name + ".hip"), "-o", out], check=True, capture_output=True, timeout=900)
    return open(out).read()


@pytest.mark.parametrize("name,kernel,mfma", [("gemm_f32", "gemm_f32_kernel", "v_mfma_f32_32x32x2_f32"),
                                              ("attention_f32", "attention_f32_kernel", "v_mfma_f32_16x16x4_f32")])
def test_new_kernels_cross_compile_without_scratch(tmp_path, name, kernel, mfma):
    isa = _isa(tmp_path, name)
    assert "scratch_" not in isa
    sizes = re.findall(r"\.private_seg_size, (\d+)", isa) + re.findall(r"\.private_segment_fixed_size: (\d+)", isa)
    assert sizes and all(int(s) == 0 for s in sizes), sizes
    assert re.search(r"^\s*\.amdhsa_kernel \S*" + kernel, isa, re.M), "kernel not emitted"
    assert mfma in isa
    assert int(re.search(r"\.vgpr_spill_count:\s+(\d+)", isa).group(1)) == 0


def _gemm(**kw):
    """fc1 of ViT-H at one hand.  Fake, never dereferenced pointers."""
    a = L.GemmArgs(X=4096, W=4096, C=4096, bias=4096, M=192, N=5120, K=1280, ldx=1280, ldw=1280, ldc=5120,
                   epilogue=L.HM_EPI_GELU, dtype=L.HM_DTYPE_F32)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_gemm_f32_rejects_bad_arguments():
    lib = L.load()
    bad = [dict(dtype=L.HM_DTYPE_F16), dict(dtype=L.HM_DTYPE_BF16), dict(X=0), dict(W=0), dict(C=0), dict(M=0), dict(N=0), dict(K=0),
           dict(K=1296, ldx=1296, ldw=1296), dict(ldx=1278), dict(ldw=1276), dict(ldc=5000), dict(ldx=1282), dict(X=8), dict(W=8),
           dict(C=2), dict(bias=2), dict(epilogue=L.HM_EPI_STORE), dict(epilogue=L.HM_EPI_RESID_LN), dict(epilogue=L.HM_EPI_SILU),
           dict(k_split=2), dict(ln_gamma=4096), dict(ln_colsum=4096), dict(out_scale=0.5),
           dict(epilogue=L.HM_EPI_RESID_F32), dict(epilogue=L.HM_EPI_RESID_F32, resid=4096, ldr=1280),
           dict(epilogue=L.HM_EPI_RESID_F32, resid=4096, ldr=5120, resid_mod=-1)]
    for kw in bad:
        assert lib.hm_gemm_f32(C.byref(_gemm(**kw)), None) == HM_ERR_ARG, kw
        assert b"hm_gemm_f32" in lib.hm_last_error_string(), kw
    assert lib.hm_gemm_f32(None, None) == HM_ERR_ARG


def test_attention_f32_rejects_bad_arguments():
    lib = L.load()
    f = C.c_float(80 ** -0.5)
    for qkv, out, B, T, H, d in ((None, P16, 1, 192, 16, 80), (P16, None, 1, 192, 16, 80), (P16, P16, 0, 192, 16, 80),
                                 (P16, P16, 1, 191, 16, 80), (P16, P16, 1, 192, 16, 64), (P16, P16, 1, 192, 0, 80),
                                 (P8, P16, 1, 192, 16, 80), (P16, P8, 1, 192, 16, 80)):
        assert lib.hm_vit_attention_f32(qkv, out, B, T, H, d, f, None) == HM_ERR_ARG
        assert b"hm_vit_attention_f32" in lib.hm_last_error_string()


def _weights(cfg, **kw):
    """An hm_hamer_weights with fake pointers (never dereferenced: every case below is refused before the first launch)."""
    v, d = cfg.vit, cfg.dec
    blocks, layers = (L.VitBlock * v.depth)(), (L.DecLayer * d.depth)()
    for b in blocks:
        for n in ("ln1_g", "ln1_b", "ln2_g", "ln2_b", "qkv_w", "proj_w", "fc1_w", "fc2_w", "qkv_b", "proj_b", "fc1_b", "fc2_b"):
            setattr(b, n, 4096)
    w = L.HamerWeights()
    w.img_h, w.img_w_full, w.win_x0, w.win_w, w.patch, w.pad = v.img_h, cfg.image_size, 32, v.img_w, v.patch, v.pad
    w.embed_dim, w.depth, w.heads, w.mlp_dim, w.vit_eps = v.embed_dim, v.depth, v.heads, v.embed_dim * v.mlp_ratio, v.ln_eps
    for n in ("patch_w", "patch_b", "pos", "last_g", "last_b", "token0", "kv_w", "head_w", "head_b"):
        setattr(w, n, 4096)
    w.blocks, w.layers = C.cast(blocks, C.POINTER(L.VitBlock)), C.cast(layers, C.POINTER(L.DecLayer))
    w.dec_dim, w.dec_depth, w.dec_heads, w.dec_dim_head, w.dec_mlp, w.dec_eps = d.dim, d.depth, d.heads, d.dim_head, d.mlp_dim, d.ln_eps
    w.dtype = L.HM_DTYPE_F32
    w._keep = (blocks, layers)
    return w, blocks, layers


def test_forward_f32_refuses_what_the_route_does_not_carry():
    lib = L.load()
    cfg = synth.tiny_config()
    outs = L.HamerOutputs(*([4096] * 8), None)

    def run(w):
        return lib.hm_hamer_forward(C.byref(w), P16, 1, C.byref(outs), P16, 1 << 40, None)

    for field in ("qkv_w8", "fc1_ws", "proj_w8", "qkv_colsum", "fc1_bias_ln", "kmean_w"):
        w, blocks, _ = _weights(cfg)
        setattr(blocks[1], field, 4096)
        assert run(w) == HM_ERR_ARG, field
        assert b"fp32" in lib.hm_last_error_string(), field
    w, blocks, _ = _weights(cfg)
    blocks[0].gelu_out_scale = 0.5
    assert run(w) == HM_ERR_ARG and b"prescale" in lib.hm_last_error_string()
    w, _, layers = _weights(cfg)
    layers[1].ca_scale_mul = 4.0
    assert run(w) == HM_ERR_ARG and b"prescale" in lib.hm_last_error_string()
    w, _, _ = _weights(cfg)
    r = (C.c_int * cfg.vit.depth)(8, 8)
    w.tome_r = C.cast(r, C.POINTER(C.c_int))
    assert run(w) == HM_ERR_ARG and b"token merging" in lib.hm_last_error_string()
    w, _, _ = _weights(cfg)
    w.range_stats = 4096
    assert run(w) == HM_ERR_ARG and b"range_stats" in lib.hm_last_error_string()
    w, _, _ = _weights(cfg)
    w.dtype = 7
    assert run(w) == HM_ERR_ARG


def test_workspace_of_the_fp32_route_holds_fp32_activations():
    """ViT-H at B = 64: qkv 189 MB and the MLP hidden 252 MB in fp32; the 16-bit layout is unchanged next to it."""
    lib = L.load()
    cfg = synth.HamerConfig()
    w, _, _ = _weights(cfg)
    n32 = lib.hm_hamer_workspace_bytes(C.byref(w), 64)
    w.dtype = L.HM_DTYPE_F16
    n16 = lib.hm_hamer_workspace_bytes(C.byref(w), 64)
    M, D = 64 * 192, 1280
    per_elem = M * (768 + D + 3 * D + D + 4 * D + cfg.dec.depth * 2 * cfg.dec.inner)      # patches, h, qkv, att, mlp, kv
    assert n32 - n16 == 2 * per_elem, (n32, n16)
    assert M * 3 * D * 4 == 188743680 and M * 4 * D * 4 == 251658240


def test_switches_and_cli_flags(monkeypatch):
    from hamer_yolo_amd import d_infer, infer
    from hamer_yolo_amd.config.hamer_config import Config, hamer_opt
    from hamer_yolo_amd.config.yolo_config import yolo_opt
    from hamer_yolo_amd.hamer.models import load_hamer
    from hamer_yolo_amd.hamer.models.hamer import HAMER
    from hamer_yolo_amd.rootnet.sar_config_stage_1 import rgb_opt
    assert Config.precise is False and hamer_opt.precise is False
    assert inspect.signature(load_hamer).parameters["precise"].default is False
    assert inspect.signature(infer.hamer_inference.__init__).parameters["precise"].default is None
    assert inspect.signature(HAMER.__init__).parameters["dtype"].default is torch.float16
    base = ["--input", "a", "--output", "b"]
    a = infer._parser().parse_args(base)
    assert a.precise is False and a.precise_hamer is False
    for opt in (hamer_opt, yolo_opt, rgb_opt):
        monkeypatch.setattr(opt, "precise", False, raising=False)
    infer.apply_precise_args(infer._parser().parse_args(base + ["--precise-hamer"]))
    assert hamer_opt.precise is True and yolo_opt.precise is False
    monkeypatch.setattr(hamer_opt, "precise", False)
    infer.apply_precise_args(infer._parser().parse_args(base + ["--precise"]))
    assert hamer_opt.precise is True and yolo_opt.precise is True and rgb_opt.precise is False      # infer.py has no RootNet
    for opt in (hamer_opt, yolo_opt):
        monkeypatch.setattr(opt, "precise", False)
    dbase = base + ["--intrinsics", "k.txt"]
    d_infer.apply_precise_args(d_infer._parser().parse_args(dbase + ["--precise-hamer"]))
    assert hamer_opt.precise is True and yolo_opt.precise is False and rgb_opt.precise is False
    monkeypatch.setattr(hamer_opt, "precise", False)
    d_infer.apply_precise_args(d_infer._parser().parse_args(dbase + ["--precise"]))
    assert hamer_opt.precise is True and yolo_opt.precise is True and rgb_opt.precise is True


def test_engine_argument_checks_need_no_device():
    """token merging / fp8 / deferred LayerNorm / prescale with fp32 operands: a ValueError that says so, before any device work."""
    from hamer_yolo_amd.engine import HamerEngine
    from hamer_yolo_amd.hamer.configs import get_config
    from hamer_yolo_amd.hamer.models.hamer import HAMER
    from hamer_yolo_amd.hamer.models.mano_wrapper import MANO
    cfg = synth.tiny_config()
    sd, mp = synth.hamer_state_dict(cfg, seed=0), synth.mano_params(seed=0)
    with pytest.raises(ValueError, match="token merging"):
        HamerEngine(sd, mp, cfg, dtype=torch.float32, token_merge=True)
    with pytest.raises(ValueError, match="token merging"):
        HamerEngine(sd, mp, cfg, dtype=torch.float32, token_merge=[8, 8])
    with pytest.raises(ValueError, match="fp8"):
        HamerEngine(sd, mp, cfg, dtype=torch.float32, fp8=True)
    with pytest.raises(ValueError, match="fold_ln"):
        HamerEngine(sd, mp, cfg, dtype=torch.float32, fold_ln=True)
    pre = {"blocks": [dict(ln1=1, q=0, k=0, v=0, ln2=0, gelu=0)] * cfg.vit.depth, "last": 0, "dec": [(0, 0)] * cfg.dec.depth}
    with pytest.raises(ValueError, match="prescale"):
        HamerEngine(sd, mp, cfg, dtype=torch.float32, prescale=pre)
    with pytest.raises(ValueError, match="token merging"):
        HAMER(get_config(None), sd, MANO.synthetic(0), dtype=torch.float32, hamer_cfg=cfg, token_merge=(8, -1))


def test_engine_packs_fp32_weights(monkeypatch):
    """Construction only (no launch): fp32 GEMM operands, HM_DTYPE_F32, the decoder's two self-attention linears unfolded."""
    from hamer_yolo_amd.engine import HamerEngine
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    cfg = synth.tiny_config()
    sd, mp = synth.hamer_state_dict(cfg, seed=0), synth.mano_params(seed=0)
    e = HamerEngine(sd, mp, cfg, device="cpu", dtype=torch.float32)
    assert e.precise and e.w.dtype == L.HM_DTYPE_F32 and not e.fold_ln and not e.fp8 and e.prescale is None and e.tome_r is None
    assert all(t.dtype in (torch.float32,) for t in e._keep if t.is_floating_point())
    by_ptr = {t.data_ptr(): t for t in e._keep}
    qkv = by_ptr[e.blocks[0].qkv_w]
    assert qkv.dtype == torch.float32 and torch.equal(qkv, sd["backbone.blocks.0.attn.qkv.weight"])
    assert e.layers[0].sa_w is None and e.layers[0].sa_v_w is not None
    assert e.blocks[0].qkv_colsum is None and e.blocks[0].qkv_w8 is None and e.blocks[0].kmean_w is None
    e16 = HamerEngine(sd, mp, cfg, device="cpu")
    assert not e16.precise and e16.w.dtype == L.HM_DTYPE_F16 and e16.layers[0].sa_w is not None
    assert {t.data_ptr(): t for t in e16._keep}[e16.blocks[0].qkv_w].dtype == torch.float16


def test_fp64_chain_is_the_fp32_oracle_in_double():
    cfg = synth.tiny_config()
    sd, mp = synth.hamer_state_dict(cfg, seed=0), synth.mano_params(seed=0)
    img = synth.normalize_crops(synth.crops_u8(2, seed0=0))
    with torch.no_grad():
        ref = R.hamer_forward(sd, mp, img, cfg)
    o32 = PC.chain_forward(sd, mp, img, cfg, dtype=torch.float32)
    assert set(o32) == set(ref)
    for k in ref:
        assert o32[k].dtype == torch.float32 and torch.equal(o32[k], ref[k]), k
    o64 = PC.chain_forward(sd, mp, img, cfg, dtype=torch.float64)
    assert torch.get_default_dtype() == torch.float32
    for k in ref:
        assert o64[k].dtype == torch.float64, k                    # no silent fp32 intermediate ends in an fp32 tensor
        if k == "focal_length":
            continue
        d = float((o64[k] - ref[k].double()).abs().max())
        assert 0.0 < d <= 2e-5, (k, d)
    v32, v64 = PC.engine_view(o32), PC.engine_view(o64)
    assert set(v32) == set(PC.ENGINE_KEYS) and v64["tokens"].shape == (2 * 192, cfg.vit.embed_dim) and v64["rotmats"].shape == (2, 16, 3, 3)
    assert all(v > 0 for v in PC.distances(v32, v64).values())
