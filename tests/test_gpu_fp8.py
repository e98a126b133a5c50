"""GPU parity of the fp8 path (BASELINE configs[4]) against the fp8-quantised oracle (oracle/fp8_ref.py).

hm_gemm_fp8 is exact up to fp32 accumulation order once both sides see the same e4m3 bytes and scales, so the
tolerances below are those of the 16-bit GEMM tests; quantisers (LayerNorm -> MXFP8, GELU -> MXFP8) must reproduce
the oracle's bytes except where a last-bit fp32 difference crosses an e4m3 rounding boundary.
"""
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exact_data as ED  # noqa: E402

from hamer_yolo_amd import lib as L
from hamer_yolo_amd import ops, synth
from oracle import fp8_ref as Q

DEV = "cuda"


def _u(name, shape, hw=1.0, seed=0, center=0.0):
    return synth.uniform(name, shape, hw, center, seed=seed)


def _operands(M, N, K, seed):
    x = _u("fx", (M, K), 2.0, seed=seed) * (1.0 + 4.0 * _u("fxr", (M, 1), 0.5, seed=seed + 1, center=0.5))   # rows of different size
    w = _u("fw", (N, K), 0.05, seed=seed + 2) * (0.2 + _u("fwr", (N, 1), 0.5, seed=seed + 3, center=0.5))
    x8, xs = Q.mx8_quantize(x)
    w8, ws = Q.quantize_weight(w)
    ref = Q.mx8_dequantize(x8, xs).double() @ Q.dequantize_weight(w8, ws).double().t()
    return x8, xs, w8, ws, ref


def test_gemm_fp8_exact_integers():
    """Hashed small-integer e4m3 values and hashed power-of-two scales (tests/exact_data.py): every product and sum is exact
    in fp32 -> bit-exact result, and no operand element or scale repeats with a period along K, M or N, which pins the operand
    and scale lane maps of v_mfma_scale_f32_16x16x128_f8f6f4 through the whole kernel (the faults this data sees are listed in
    tests/test_exact_data_host.py)."""
    for (M, N, K) in ED.GEMM_FP8:
        x8, xs, w8, ws, xi, wi = ED.fp8_case(M, N, K)
        ref = (Q.mx8_dequantize(x8, xs).double() @ (wi.double() * ws.double()[:, None]).t())
        assert torch.equal(ref, ED.fp8_reference(xi, xs, wi, ws))                  # the oracle's dequantiser and the plain statement agree
        out = ops.gemm_fp8(x8.to(DEV), xs.to(DEV), w8.to(DEV), ws.to(DEV), None, L.HM_EPI_RESID_F32,
                           resid=torch.zeros(M, N, device=DEV))
        ED.assert_exact(out.cpu().double(), ref, (M, N, K))


@pytest.mark.parametrize("M,N,K", [(384, 3840, 1280), (768, 1280, 5120), (1040, 320, 256), (16, 64, 128)])
def test_gemm_fp8_epilogues(M, N, K):
    x8, xs, w8, ws, ref = _operands(M, N, K, seed=M + N)
    bias, resid = _u("fb", (N,), 0.5, seed=5), _u("fr", (M, N), 1.0, seed=6)
    a = (x8.to(DEV), xs.to(DEV), w8.to(DEV), ws.to(DEV), bias.to(DEV))
    scale = ref.abs().max().item()
    o = ops.gemm_fp8(*a, L.HM_EPI_RESID_F32, resid=resid.to(DEV)).cpu().double()
    np.testing.assert_allclose(o.numpy(), (ref + bias.double() + resid.double()).numpy(), atol=2e-6 * scale * math.sqrt(K), rtol=1e-5)
    o = ops.gemm_fp8(*a, L.HM_EPI_STORE).cpu().float()
    np.testing.assert_allclose(o.numpy(), (ref + bias.double()).float().numpy(), atol=1e-5 * scale * math.sqrt(K), rtol=2 ** -7)
    # GELU -> MXFP8: bytes and scales against the oracle quantiser applied to the fp64 result
    o8, os_ = ops.gemm_fp8(*a, L.HM_EPI_GELU_MX8)
    g = F.gelu((ref + bias.double()).float())
    r8, rs = Q.mx8_quantize(g)
    same_scale = (os_.cpu() == rs).float().mean().item()
    assert same_scale > 0.995, same_scale
    d_k, d_r = Q.mx8_dequantize(o8.cpu(), os_.cpu()), Q.mx8_dequantize(r8, rs)
    err = (d_k - d_r).abs()
    blockmax = d_r.abs().reshape(M, N // 32, 32).amax(-1, keepdim=True).expand(M, N // 32, 32).reshape(M, N)
    assert (err <= blockmax * 2.0 ** -3 + 1e-6).all()              # never more than one e4m3 step of the block's range
    assert (err == 0).float().mean().item() > 0.99


@pytest.mark.parametrize("D", [1280, 320, 32, 768, 1536, 2048])      # MAXJ 5, 2, 2 (one 8-lane group), 5, 8, 8
def test_layernorm_mx8(D):
    M = 520
    x = _u("lx", (M, D), 2.0, seed=D) + _u("lxr", (M, 1), 3.0, seed=D + 1)
    gamma, beta = _u("lg", (D,), 0.3, seed=3, center=1.0), _u("lb", (D,), 0.2, seed=4)
    o8, os_ = ops.layernorm_mx8(x.to(DEV), gamma.to(DEV), beta.to(DEV), 1e-6)
    y = F.layer_norm(x, (D,), gamma, beta, 1e-6)
    r8, rs = Q.mx8_quantize(y)
    assert (os_.cpu() == rs).float().mean().item() > 0.995
    d_k, d_r = Q.mx8_dequantize(o8.cpu(), os_.cpu()), Q.mx8_dequantize(r8, rs)
    assert not torch.isnan(d_k).any()
    err = (d_k - d_r).abs()
    blockmax = d_r.abs().reshape(M, D // 32, 32).amax(-1, keepdim=True).expand(M, D // 32, 32).reshape(M, D)
    assert (err <= blockmax * 2.0 ** -3 + 1e-6).all()
    assert (err == 0).float().mean().item() > 0.99
    # and the quantised rows still are the LayerNorm to e4m3 precision
    assert ((d_k - y).abs() <= blockmax * 2.0 ** -4 + 1e-6).float().mean().item() > 0.999


@pytest.mark.parametrize("grid", [0, 8, 40])
def test_gemm_fp8_persistent_kernel_is_bit_identical_to_one_tile_kernel(grid):
    """qkv / fc1 shapes of whole 256 x 256 tiles run in the persistent kernel (several tiles per workgroup, the next tile's
    first K-step in flight under the epilogue, hand-counted waits).  Same MFMA order, same epilogue arithmetic: the bytes
    must equal the one-tile kernel's, for one tile per workgroup (default grid) and for many (HM_OPT_FP8P_GRID)."""
    M, N, K = 2304, 3840, 1280                       # 9 x 15 tiles
    x8, xs, w8, ws, _ = _operands(M, N, K, seed=11)
    bias = _u("fb", (N,), 0.5, seed=5)
    a = (x8.to(DEV), xs.to(DEV), w8.to(DEV), ws.to(DEV), bias.to(DEV))
    resid = _u("fr", (M, N), 1.0, seed=6).to(DEV)
    with L.option(L.HM_OPT_FP8_ONE_TILE, 1):
        ref_store = ops.gemm_fp8(*a, L.HM_EPI_STORE)
        ref8, refs = ops.gemm_fp8(*a, L.HM_EPI_GELU_MX8)
        ref_res = ops.gemm_fp8(*a, L.HM_EPI_RESID_F32, resid=resid)
    # the persistent residual epilogue is opt-in (not faster), still pinned here
    with L.option(L.HM_OPT_FP8P_GRID, grid), L.option(L.HM_OPT_FP8P_RESID, 1):
        for _ in range(2):
            out = ops.gemm_fp8(*a, L.HM_EPI_STORE)
            o8, os_ = ops.gemm_fp8(*a, L.HM_EPI_GELU_MX8)
            assert torch.equal(out.view(torch.int16), ref_store.view(torch.int16))
            assert torch.equal(o8, ref8) and torch.equal(os_, refs)
            # fp32 residual epilogue (proj / fc2): residual rows prefetched into registers by untracked loads, counted waits
            assert torch.equal(ops.gemm_fp8(*a, L.HM_EPI_RESID_F32, resid=resid), ref_res)
            x_inplace = resid.clone()                          # the forward updates the residual stream in place
            ops.gemm_fp8(*a, L.HM_EPI_RESID_F32, resid=x_inplace, out=x_inplace)
            assert torch.equal(x_inplace, ref_res)


def test_gemm_fp8_rejects_bad_arguments():
    x8 = torch.zeros(16, 128, device=DEV, dtype=torch.uint8)
    xs = torch.zeros(4, 16, device=DEV, dtype=torch.uint8)
    w8 = torch.zeros(64, 128, device=DEV, dtype=torch.uint8)
    ws = torch.ones(64, device=DEV)
    ops.gemm_fp8(x8, xs, w8, ws)                                   # smallest legal problem
    with pytest.raises(L.HipLibraryError):
        ops.gemm_fp8(x8[:, :64].contiguous(), xs[:2].contiguous(), w8[:, :64].contiguous(), ws)      # K % 128 != 0
    with pytest.raises(L.HipLibraryError):
        ops.gemm_fp8(x8, xs, w8[:48].contiguous(), ws[:48].contiguous())                             # N % 64 != 0


def test_vith_forward_fp8_vs_fp8_oracle(golden_dir):
    """Full ViT-H/16 + decoder + MANO with qkv / fc1 / fc2 on the fp8 MFMA against the oracle run with the same
    quantisation (emu="fp8"); the distance to the fp32 reference golden is reported by the looser second bound."""
    import os
    from hamer_yolo_amd.engine import HamerEngine
    from oracle import hamer_ref as R
    g = np.load(os.path.join(golden_dir, "hamer_vith.npz"))
    cfg = synth.HamerConfig()
    sd = synth.hamer_state_dict(cfg, seed=int(g["seed"]), device="cuda")
    mp = synth.mano_params(seed=0)
    eng = HamerEngine(sd, mp, cfg, fp8=True)
    assert eng.fp8
    img = synth.normalize_crops(synth.crops_u8(2, seed0=int(g["crop_seed0"])))
    out = eng.forward(img.cuda())
    torch.cuda.synchronize()
    with torch.no_grad():
        ref = R.hamer_forward({k: v.cpu() for k, v in sd.items()}, mp, img, cfg, emu="fp8")
    for k in ("pose6d", "betas", "pred_cam"):
        assert torch.isfinite(out[k]).all()
    d_pose = (out["pose6d"].cpu() - ref["pose6d"]).abs().max().item()
    d_vert = (out["pred_vertices"].cpu() - ref["pred_vertices"]).abs().max().item()
    g_pose = np.abs(out["pose6d"].cpu().numpy() - g["pose6d"][:2]).max()
    # distance of the fp8 configuration from the fp32 reference path, mesh included (the accuracy cost of configs[4])
    v32, _ = R.mano_forward(mp, torch.from_numpy(g["betas"][:2]), torch.from_numpy(g["rotmats"][:2]))
    g_vert = (out["pred_vertices"].cpu() - v32).abs().max().item()
    g_rot = np.abs(out["rotmats"].cpu().numpy() - g["rotmats"][:2]).max()
    print(f"fp8: |pose6d - fp8 oracle| {d_pose:.2e}  |verts - fp8 oracle| {d_vert:.2e}  |pose6d - fp32 reference| {g_pose:.2e}  "
          f"|rotmats - fp32 reference| {g_rot:.2e}  |verts - fp32 reference| {g_vert:.2e}")
    import json, os as _os
    try:
        _d = _os.path.join(_os.path.dirname(_os.path.dirname(_os.path.abspath(__file__))), "gpurun_out")
        _os.makedirs(_d, exist_ok=True)
        with open(_os.path.join(_d, "parity_report.jsonl"), "a") as f:
            f.write(json.dumps({"test": "vith_fp8", "pose6d_vs_fp8_oracle": d_pose, "verts_vs_fp8_oracle": d_vert,
                                "pose6d_vs_fp32_reference": float(g_pose), "rotmats_vs_fp32_reference": float(g_rot),
                                "verts_vs_fp32_reference": g_vert}) + "\n")
    except OSError:
        pass
    assert g_vert < 5e-3
    # same quantisation on both sides: what is left are e4m3 rounding flips triggered by fp32 summation order
    assert d_pose < 1e-2 and d_vert < 2e-3
    # against the fp32 reference modules: e4m3 has 3 mantissa bits; this is the accuracy cost of configs[4], not a parity bar
    assert g_pose < 5e-2


def test_fp8_batch256_properties():
    """BASELINE configs[4] at its full size (B = 256, M = 49152 rows through gemm_fp8_kernel): finite, rotations orthonormal,
    every crop's result independent of its position in the batch (the 256 crops are 4 different ones repeated: equal rows
    bit for bit), and equal to what a B = 4 forward gives for the same crops up to the summation-order noise of the small-M
    tile path."""
    from hamer_yolo_amd.engine import HamerEngine
    cfg = synth.HamerConfig()
    sd = synth.hamer_state_dict(cfg, seed=0, device="cuda")
    eng = HamerEngine(sd, synth.mano_params(seed=0), cfg, fp8=True)
    img4 = synth.normalize_crops(synth.crops_u8(4, seed0=0)).cuda()
    o4 = {k: v.clone() for k, v in eng.forward(img4).items()}
    o = eng.forward(img4.repeat(64, 1, 1, 1))
    torch.cuda.synchronize()
    for k in ("pose6d", "betas", "pred_cam", "pred_vertices", "pred_keypoints_3d", "rotmats"):
        v = o[k]
        assert v.shape[0] == 256 and torch.isfinite(v).all(), k
        assert torch.equal(v[:4], v[252:256]) and torch.equal(v[4:8], v[128:132]), k
    r = o["rotmats"]
    np.testing.assert_allclose((r @ r.transpose(-1, -2)).cpu().numpy(), torch.eye(3).expand_as(r).numpy(), atol=1e-5)
    assert float((o["pose6d"][:4] - o4["pose6d"]).abs().max()) < 2e-2          # e4m3 rounding flips under another summation order
    assert float((o["pred_vertices"][:4] - o4["pred_vertices"]).abs().max()) < 5e-3


def test_vit_attention_mx8_matches_16bit_kernel_then_quantised():
    """hm_vit_attention_mx8 = the attention of hm_vit_attention, taken before the 16-bit rounding, as MXFP8 with every head
    widened to 96 columns: dequantised it must equal the bf16 kernel's output to e4m3 precision, the pad columns are
    exact zeros and the scales are those of the oracle quantiser applied to the padded fp32 attention."""
    B, H, T, d = 3, 16, 192, 80
    qkv = (_u("aq", (B * T, 3 * H * d), 1.5, seed=11)).to(torch.bfloat16)
    ref16 = ops.vit_attention(qkv.to(DEV), B, T, H, d, d ** -0.5).float().cpu()                 # (B*T, H*80)
    o8, os_ = ops.vit_attention_mx8(qkv.to(DEV), B, T, H, d, d ** -0.5)
    assert o8.shape == (B * T, H * 96) and os_.shape == (H * 3, B * T)
    deq = Q.mx8_dequantize(o8.cpu(), os_.cpu()).reshape(B * T, H, 96)
    assert (deq[:, :, 80:] == 0).all() and (o8.cpu().reshape(B * T, H, 96)[:, :, 80:] == 0).all()
    got = deq[:, :, :80].reshape(B * T, H * 80)
    blockmax = torch.zeros(B * T, H, 96)
    blockmax[:, :, :80] = ref16.reshape(B * T, H, 80).abs()
    blockmax = blockmax.reshape(B * T, H * 3, 32).amax(-1, keepdim=True).expand(-1, -1, 32).reshape(B * T, H, 96)[:, :, :80].reshape(B * T, H * 80)
    assert ((got - ref16).abs() <= blockmax * 2.0 ** -3 + 1e-6).all()
    # scales: quantise the (bf16-rounded) reference the same way; a scale may differ only where the block maximum sits on a
    # power-of-two boundary after the bf16 rounding
    pad = torch.zeros(B * T, H, 96)
    pad[:, :, :80] = ref16.reshape(B * T, H, 80)
    _, rs = Q.mx8_quantize(pad.reshape(B * T, H * 96))
    assert (os_.cpu() == rs).float().mean().item() > 0.99
