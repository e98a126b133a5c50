"""Thin tensor-level wrappers over the C ABI (one per exported kernel).

Tensors are PyTorch-ROCm tensors used as device buffers; every function checks shapes on the
host before handing raw pointers to the library, and raises on any library error.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from . import lib as L

_DT = {torch.bfloat16: L.HM_DTYPE_BF16, torch.float16: L.HM_DTYPE_F16}


def _dt(t: torch.Tensor) -> int:
    if t.dtype not in _DT:
        raise TypeError(f"16-bit operand expected (bfloat16/float16), got {t.dtype}")
    return _DT[t.dtype]


def _dev(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise L.HipLibraryError("libhamer_hip kernels take device tensors; there is no CPU path")


def gemm(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, epilogue: int = L.HM_EPI_STORE,
         resid: Optional[torch.Tensor] = None, resid_mod: int = 0, out: Optional[torch.Tensor] = None,
         ln_gamma: Optional[torch.Tensor] = None, ln_xg: Optional[torch.Tensor] = None,
         ln_stats: Optional[torch.Tensor] = None, ln_colsum: Optional[torch.Tensor] = None, k_split: int = 0) -> torch.Tensor:
    """out = epilogue(x @ w.T + bias); x (M,K), w (N,K) 16-bit row-major.  Deferred LayerNorm: HM_EPI_RESID_LN also
    fills ln_xg (M,N) 16-bit = out * ln_gamma and ln_stats (N/64, M, 2); HM_EPI_LN_STORE / HM_EPI_LN_GELU read
    ln_stats (M, 2) = ln_finalize(partials) and ln_colsum (N,)."""
    _dev(x, w, bias, resid, out, ln_gamma, ln_xg, ln_stats, ln_colsum)
    M, K = x.shape
    N = w.shape[0]
    assert w.shape[1] == K and x.stride(1) == 1 and w.stride(1) == 1 and x.dtype == w.dtype
    f32_out = epilogue in (L.HM_EPI_RESID_F32, L.HM_EPI_F32, L.HM_EPI_RESID_LN)
    if epilogue == L.HM_EPI_RESID_LN:
        assert ln_xg.shape == (M, N) and ln_xg.is_contiguous() and ln_xg.dtype == x.dtype
        assert ln_stats.shape == (N // 64, M, 2) and ln_stats.is_contiguous() and ln_gamma.shape == (N,)
    if epilogue in (L.HM_EPI_LN_STORE, L.HM_EPI_LN_GELU):
        assert ln_stats.shape == (M, 2) and ln_stats.is_contiguous() and ln_colsum.shape == (N,)
    if k_split > 1:                      # HM_EPI_F32 split-K: out is (k_split, M, N) partial products
        assert epilogue == L.HM_EPI_F32 and bias is None
        if out is None:
            out = torch.empty(k_split, M, N, device=x.device, dtype=torch.float32)
        assert out.shape == (k_split, M, N) and out.is_contiguous()
        a = L.GemmArgs(L.ptr(x), L.ptr(w), L.ptr(out), None, None, M, N, K, x.stride(0), w.stride(0), N, 0, 0, epilogue,
                       _dt(x), None, None, None, None, k_split)
        L.check(L.load().hm_gemm(C.byref(a), L.current_stream()), "hm_gemm")
        return out
    if out is None:
        out = torch.empty(M, N, device=x.device, dtype=torch.float32 if f32_out else x.dtype)
    assert out.shape == (M, N) and out.stride(1) == 1
    a = L.GemmArgs(L.ptr(x), L.ptr(w), L.ptr(out), L.ptr(bias), L.ptr(resid), M, N, K, x.stride(0), w.stride(0),
                   out.stride(0), resid.stride(0) if resid is not None else 0, resid_mod, epilogue, _dt(x),
                   L.ptr(ln_gamma), L.ptr(ln_xg), L.ptr(ln_stats), L.ptr(ln_colsum), 0)
    L.check(L.load().hm_gemm(C.byref(a), L.current_stream()), "hm_gemm")
    return out


def gemm_f32(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, epilogue: int = L.HM_EPI_F32,
             resid: Optional[torch.Tensor] = None, resid_mod: int = 0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """hm_gemm_f32 (the precise route): out (M,N) fp32 = epilogue(x @ w.T + bias), x (M,K) and w (N,K) fp32 row-major;
    epilogue HM_EPI_F32, HM_EPI_GELU or HM_EPI_RESID_F32 (+ resid[m % resid_mod], which may be `out` itself)."""
    _dev(x, w, bias, resid, out)
    M, K = x.shape
    N = w.shape[0]
    assert w.shape[1] == K and x.stride(1) == 1 and w.stride(1) == 1 and x.dtype == w.dtype == torch.float32
    if out is None:
        out = torch.empty(M, N, device=x.device, dtype=torch.float32)
    assert out.shape == (M, N) and out.stride(1) == 1 and out.dtype == torch.float32
    a = L.GemmArgs(L.ptr(x), L.ptr(w), L.ptr(out), L.ptr(bias), L.ptr(resid), M, N, K, x.stride(0), w.stride(0),
                   out.stride(0), resid.stride(0) if resid is not None else 0, resid_mod, epilogue, L.HM_DTYPE_F32)
    L.check(L.load().hm_gemm_f32(C.byref(a), L.current_stream()), "hm_gemm_f32")
    return out


def vit_attention_f32(qkv: torch.Tensor, B: int, tokens: int, heads: int, head_dim: int, scale: float) -> torch.Tensor:
    """hm_vit_attention_f32 (the precise route): qkv (B*tokens, 3*heads*head_dim) fp32 -> (B*tokens, heads*head_dim) fp32."""
    _dev(qkv)
    assert qkv.dtype == torch.float32 and qkv.is_contiguous() and qkv.shape == (B * tokens, 3 * heads * head_dim)
    out = torch.empty(B * tokens, heads * head_dim, device=qkv.device, dtype=torch.float32)
    L.check(L.load().hm_vit_attention_f32(L.ptr(qkv), L.ptr(out), B, tokens, heads, head_dim, scale, L.current_stream()),
            "hm_vit_attention_f32")
    return out


def layernorm_accum(x: torch.Tensor, partials: torch.Tensor, bias: Optional[torch.Tensor], gamma: torch.Tensor,
                    beta: torch.Tensor, eps: float, out_dtype=torch.bfloat16) -> torch.Tensor:
    """x (M,D) f32 += bias + partials.sum(0) in place (partials (S,M,D) from gemm(k_split=S)); returns LayerNorm(x)."""
    _dev(x, partials, bias, gamma, beta)
    M, D = x.shape
    assert x.dtype == torch.float32 and x.is_contiguous() and partials.shape[1:] == (M, D) and partials.is_contiguous()
    out = torch.empty(M, D, device=x.device, dtype=out_dtype)
    code = L.HM_OUT_F32 if out_dtype == torch.float32 else _DT[out_dtype]
    L.check(L.load().hm_layernorm_accum(L.ptr(x), L.ptr(partials), partials.shape[0], L.ptr(bias), L.ptr(gamma), L.ptr(beta),
                                        L.ptr(out), code, M, D, eps, L.current_stream()), "hm_layernorm_accum")
    return out


def layernorm_mx8(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float):
    """LayerNorm -> MXFP8: (out8 (M,D) uint8 of e4m3 bytes, scales (D/32, M) uint8 E8M0)."""
    _dev(x, gamma, beta)
    M, D = x.shape
    assert x.dtype == torch.float32 and x.is_contiguous()
    out8 = torch.empty(M, D, device=x.device, dtype=torch.uint8)
    scales = torch.empty(D // 32, M, device=x.device, dtype=torch.uint8)
    L.check(L.load().hm_layernorm_mx8(L.ptr(x), L.ptr(gamma), L.ptr(beta), L.ptr(out8), L.ptr(scales), M, D, eps,
                                      L.current_stream()), "hm_layernorm_mx8")
    return out8, scales


def gemm_fp8(x8: torch.Tensor, x_scales: torch.Tensor, w8: torch.Tensor, w_scale: torch.Tensor,
             bias: Optional[torch.Tensor] = None, epilogue: int = L.HM_EPI_STORE, resid: Optional[torch.Tensor] = None,
             out: Optional[torch.Tensor] = None):
    """epilogue(dequant(x8, x_scales) @ (dequant(w8) * w_scale).T + bias).  x8 (M,K) / w8 (N,K) uint8 e4m3 bytes, x_scales
    (K/32, M) uint8 E8M0, w_scale (N,) f32.  HM_EPI_STORE -> bf16; HM_EPI_RESID_F32 -> f32 (+resid); HM_EPI_GELU_MX8 ->
    (uint8 (M,N), scales (N/32, M))."""
    _dev(x8, x_scales, w8, w_scale, bias, resid, out)
    M, K = x8.shape
    N = w8.shape[0]
    assert x8.dtype == torch.uint8 and w8.dtype == torch.uint8 and w8.shape[1] == K and x8.stride(1) == 1 and w8.stride(1) == 1
    assert x_scales.shape == (K // 32, M) and x_scales.is_contiguous() and w_scale.shape == (N,)
    out_scales = None
    if out is None:
        dt = {L.HM_EPI_STORE: torch.bfloat16, L.HM_EPI_RESID_F32: torch.float32, L.HM_EPI_GELU_MX8: torch.uint8}[epilogue]
        out = torch.empty(M, N, device=x8.device, dtype=dt)
    if epilogue == L.HM_EPI_GELU_MX8:
        out_scales = torch.empty(N // 32, M, device=x8.device, dtype=torch.uint8)
    a = L.GemmFp8Args(L.ptr(x8), L.ptr(x_scales), L.ptr(w8), L.ptr(w_scale), L.ptr(out), L.ptr(bias), L.ptr(resid),
                      L.ptr(out_scales), M, N, K, x8.stride(0), w8.stride(0), out.stride(0),
                      resid.stride(0) if resid is not None else 0, epilogue, L.HM_DTYPE_BF16)
    L.check(L.load().hm_gemm_fp8(C.byref(a), L.current_stream()), "hm_gemm_fp8")
    return (out, out_scales) if epilogue == L.HM_EPI_GELU_MX8 else out


def ln_finalize(partials: torch.Tensor, eps: float) -> torch.Tensor:
    """(D/64, M, 2) partial (sum, sum of squares) -> (M, 2) (mean, rstd)."""
    _dev(partials)
    P, M, _ = partials.shape
    out = torch.empty(M, 2, device=partials.device, dtype=torch.float32)
    L.check(L.load().hm_ln_finalize(L.ptr(partials), L.ptr(out), M, P * 64, eps, L.current_stream()), "hm_ln_finalize")
    return out


def layernorm(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float, out_dtype=torch.bfloat16) -> torch.Tensor:
    _dev(x, gamma, beta)
    M, D = x.shape
    assert x.dtype == torch.float32 and x.is_contiguous()
    out = torch.empty(M, D, device=x.device, dtype=out_dtype)
    code = L.HM_OUT_F32 if out_dtype == torch.float32 else _DT[out_dtype]
    L.check(L.load().hm_layernorm(L.ptr(x), L.ptr(gamma), L.ptr(beta), L.ptr(out), code, M, D, eps, L.current_stream()),
            "hm_layernorm")
    return out


def _out_rows(out: Optional[torch.Tensor], rows: int, cols: int, dtype, device) -> torch.Tensor:
    """The caller's output buffer (its first `rows` rows are written; it may be longer) or a fresh one."""
    if out is None:
        return torch.empty(rows, cols, device=device, dtype=dtype)
    assert out.dim() == 2 and out.shape[0] >= rows and out.shape[1] == cols and out.dtype == dtype and out.is_contiguous()
    return out


def vit_attention(qkv: torch.Tensor, B: int, tokens: int, heads: int, head_dim: int, scale: float,
                  out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out: optional (>= B*tokens, heads*head_dim) buffer of qkv's dtype to write into (returned as given)."""
    _dev(qkv, out)
    assert qkv.shape == (B * tokens, 3 * heads * head_dim) and qkv.is_contiguous()
    out = _out_rows(out, B * tokens, heads * head_dim, qkv.dtype, qkv.device)
    L.check(L.load().hm_vit_attention(L.ptr(qkv), L.ptr(out), B, tokens, heads, head_dim, scale, _dt(qkv),
                                      L.current_stream()), "hm_vit_attention")
    return out


def vit_attention_mx8(qkv: torch.Tensor, B: int, tokens: int, heads: int, head_dim: int, scale: float,
                      out8: Optional[torch.Tensor] = None, scales: Optional[torch.Tensor] = None):
    """Attention with MXFP8 output: (out8 (B*tokens, heads*96) uint8, scales (heads*3, B*tokens) uint8).  out8 / scales:
    optional buffers to write into (out8 may have more rows; the scale rows have pitch B*tokens, so `scales` is exact)."""
    _dev(qkv, out8, scales)
    assert qkv.shape == (B * tokens, 3 * heads * head_dim) and qkv.is_contiguous() and qkv.dtype == torch.bfloat16
    out8 = _out_rows(out8, B * tokens, heads * 96, torch.uint8, qkv.device)
    if scales is None:
        scales = torch.empty(heads * 3, B * tokens, device=qkv.device, dtype=torch.uint8)
    assert scales.shape == (heads * 3, B * tokens) and scales.dtype == torch.uint8 and scales.is_contiguous()
    L.check(L.load().hm_vit_attention_mx8(L.ptr(qkv), L.ptr(out8), L.ptr(scales), B, tokens, heads, head_dim, scale,
                                          L.current_stream()), "hm_vit_attention_mx8")
    return out8, scales


def tome_attention(qkv: torch.Tensor, size: Optional[torch.Tensor], B: int, tokens: int, heads: int, head_dim: int,
                   scale: float, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ToMeAttention core: softmax(scale q k^T + log(size)) v for any tokens <= 192; size (B*tokens,) f32 or None.
    out: optional (>= B*tokens, heads*head_dim) buffer of qkv's dtype to write into (returned as given)."""
    _dev(qkv, size, out)
    assert qkv.shape == (B * tokens, 3 * heads * head_dim) and qkv.is_contiguous()
    assert size is None or (size.shape == (B * tokens,) and size.dtype == torch.float32 and size.is_contiguous())
    out = _out_rows(out, B * tokens, heads * head_dim, qkv.dtype, qkv.device)
    L.check(L.load().hm_tome_attention(L.ptr(qkv), L.ptr(size), L.ptr(out), B, tokens, heads, head_dim, scale, _dt(qkv),
                                       L.current_stream()), "hm_tome_attention")
    return out


def tome_merge(qkv: torch.Tensor, x: torch.Tensor, size: Optional[torch.Tensor], B: int, tokens: int, r: int, heads: int,
               head_dim: int):
    """Matching on the head-averaged keys of `qkv` + size-weighted merge of the fp32 stream x (B*tokens, D):
    returns (x_out (B*(tokens-r), D), size_out (B*(tokens-r),), index (B, 3, 96) int32 = unm | src | dst)."""
    _dev(qkv, x, size)
    D = x.shape[1]
    assert x.shape[0] == B * tokens and x.dtype == torch.float32 and x.is_contiguous() and qkv.is_contiguous()
    xo = torch.empty(B * (tokens - r), D, device=x.device, dtype=torch.float32)
    so = torch.empty(B * (tokens - r), device=x.device, dtype=torch.float32)
    metric = torch.empty(B * tokens * head_dim, device=x.device, dtype=torch.float32)
    index = torch.zeros(L.load().hm_tome_index_bytes(B) // 4, device=x.device, dtype=torch.int32)
    L.check(L.load().hm_tome_merge(L.ptr(qkv), L.ptr(x), L.ptr(size), L.ptr(xo), L.ptr(so), L.ptr(metric), L.ptr(index), B, tokens, r,
                                   heads, head_dim, D, _dt(qkv), L.current_stream()), "hm_tome_merge")
    return xo, so, index.view(B, 3, -1), metric.view(B, tokens, head_dim)


def tome_merge_metric(metric: torch.Tensor, lo_off: int, x: torch.Tensor, size: Optional[torch.Tensor], B: int, tokens: int, r: int,
                      x_out: Optional[torch.Tensor] = None, size_out: Optional[torch.Tensor] = None,
                      index: Optional[torch.Tensor] = None):
    """hm_tome_merge_metric: matching on a given fp32 metric + size-weighted merge of the fp32 stream x (B*tokens, D).
    metric: (B*tokens, >= 80) rows of any stride (taken from the tensor); lo_off > 0: the value is column d + column
    lo_off + d.  x_out (>= B*(tokens-r), D), size_out (>= B*(tokens-r),) and index (B*3*96 int32) may be given (written in
    place, further rows untouched).  Returns (x_out, size_out, index (B, 3, 96) = unm | src | dst)."""
    _dev(metric, x, size, x_out, size_out, index)
    D = x.shape[1]
    rows = B * (tokens - r)
    assert metric.dtype == torch.float32 and metric.dim() == 2 and metric.shape[0] == B * tokens and metric.stride(1) == 1
    assert metric.shape[1] >= (lo_off + 80 if lo_off else 80)
    assert x.shape[0] == B * tokens and x.dtype == torch.float32 and x.is_contiguous()
    assert size is None or (size.shape == (B * tokens,) and size.dtype == torch.float32 and size.is_contiguous())
    x_out = _out_rows(x_out, rows, D, torch.float32, x.device)
    if size_out is None:
        size_out = torch.empty(rows, device=x.device, dtype=torch.float32)
    assert size_out.dim() == 1 and size_out.shape[0] >= rows and size_out.dtype == torch.float32 and size_out.is_contiguous()
    words = L.load().hm_tome_index_bytes(B) // 4
    if index is None:
        index = torch.zeros(words, device=x.device, dtype=torch.int32)
    assert index.numel() == words and index.dtype == torch.int32 and index.is_contiguous()
    L.check(L.load().hm_tome_merge_metric(L.ptr(metric), metric.stride(0), lo_off, L.ptr(x), L.ptr(size), L.ptr(x_out), L.ptr(size_out),
                                          L.ptr(index), B, tokens, r, D, L.current_stream()), "hm_tome_merge_metric")
    return x_out, size_out, index.view(B, 3, -1)


def patch_im2col(img: torch.Tensor, x0: int, win_w: int, patch: int, pad: int, dtype=torch.bfloat16) -> torch.Tensor:
    _dev(img)
    B, Cc, H, Wf = img.shape
    assert Cc == 3 and img.dtype == torch.float32 and img.is_contiguous()
    gh, gw = (H + 2 * pad - patch) // patch + 1, (win_w + 2 * pad - patch) // patch + 1
    out = torch.empty(B * gh * gw, 3 * patch * patch, device=img.device, dtype=dtype)
    L.check(L.load().hm_patch_im2col(L.ptr(img), L.ptr(out), B, H, Wf, x0, win_w, patch, pad, _DT[dtype],
                                     L.current_stream()), "hm_patch_im2col")
    return out


def linear_f32(x: torch.Tensor, w: torch.Tensor, bias=None, resid=None, act: int = 0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """hm_linear_f32: out (M,N) fp32 = act(x @ w.T + bias) (+ resid), act 1 = GELU; x (M,K), w (N,K), resid and out row-major
    with any row stride.  out: optional buffer to write into (returned as given); it may be `resid` itself (x += ...)."""
    _dev(x, w, bias, resid, out)
    M, K = x.shape
    N = w.shape[0]
    if out is None:
        out = torch.empty(M, N, device=x.device, dtype=torch.float32)
    assert out.shape == (M, N) and out.stride(1) == 1 and out.dtype == torch.float32
    L.check(L.load().hm_linear_f32(L.ptr(x), x.stride(0), L.ptr(w), w.stride(0), L.ptr(bias), L.ptr(resid),
                                   resid.stride(0) if resid is not None else 0, L.ptr(out), out.stride(0), M, N, K, act,
                                   L.current_stream()), "hm_linear_f32")
    return out


def cross_attention(q: torch.Tensor, kv: torch.Tensor, k_off: int, v_off: int, B: int, tokens: int, heads: int,
                    dim_head: int, scale: float) -> torch.Tensor:
    """kv: 16-bit, or fp32 (the precise route: HM_DTYPE_F32)."""
    _dev(q, kv)
    out = torch.empty(B, heads * dim_head, device=q.device, dtype=torch.float32)
    code = L.HM_DTYPE_F32 if kv.dtype == torch.float32 else _dt(kv)
    L.check(L.load().hm_cross_attention(L.ptr(q), L.ptr(kv), kv.stride(0), k_off, v_off, L.ptr(out), B, tokens, heads,
                                        dim_head, scale, code, L.current_stream()), "hm_cross_attention")
    return out


def mano_model_struct(mp: dict) -> L.ManoModel:
    return L.ManoModel(L.ptr(mp["v_template"]), L.ptr(mp["shapedirs"]), L.ptr(mp["posedirs"]), L.ptr(mp["J_regressor"]),
                       L.ptr(mp["lbs_weights"]), int(mp["v_template"].shape[0]))


def mano_forward(mp: dict, pose6d: torch.Tensor, betas: torch.Tensor, cam: torch.Tensor, focal: float = 5000.0,
                 image_size: float = 256.0) -> dict:
    """mp: device fp32 tensors keyed like synth.mano_params()."""
    _dev(pose6d, betas, cam, *[mp[k] for k in ("v_template", "shapedirs", "posedirs", "J_regressor", "lbs_weights")])
    B, V, dev = pose6d.shape[0], mp["v_template"].shape[0], pose6d.device
    o = {
        "rotmats": torch.empty(B, 16, 3, 3, device=dev), "verts": torch.empty(B, V, 3, device=dev),
        "joints": torch.empty(B, 21, 3, device=dev), "cam_t": torch.empty(B, 3, device=dev),
        "kp2d": torch.empty(B, 21, 2, device=dev),
    }
    m = mano_model_struct(mp)
    L.check(L.load().hm_mano_forward(C.byref(m), L.ptr(pose6d), L.ptr(betas), L.ptr(cam), L.ptr(o["rotmats"]),
                                     L.ptr(o["verts"]), L.ptr(o["joints"]), L.ptr(o["cam_t"]), L.ptr(o["kp2d"]), B,
                                     focal, image_size, L.current_stream()), "hm_mano_forward")
    return o


def crop_boxes(boxes, P: int = 256) -> torch.Tensor:
    """boxes: iterable of (cx, cy, size, flip) -> uint8 host tensor holding hm_crop_box records."""
    lib = L.load()
    arr = (L.CropBox * len(boxes))()
    for i, (cx, cy, size, flip) in enumerate(boxes):
        L.check(lib.hm_crop_box_from_bbox(float(cx), float(cy), float(size), int(bool(flip)), P, C.byref(arr[i])),
                "hm_crop_box_from_bbox")
    return torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).clone()


def crop_batch(frame: torch.Tensor, boxes_rec: torch.Tensor, mean, std, P: int = 256, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """frame (H,W,3) uint8 BGR on device; boxes_rec: device uint8 tensor of hm_crop_box records.  ``out``: a contiguous
    (B,3,P,P) fp32 slice to fill (all hands of several frames land in one batch tensor)."""
    _dev(frame, boxes_rec, out)
    H, W, _ = frame.shape
    B = boxes_rec.numel() // C.sizeof(L.CropBox)
    if out is None:
        out = torch.empty(B, 3, P, P, device=frame.device, dtype=torch.float32)
    assert out.shape == (B, 3, P, P) and out.dtype == torch.float32 and out.is_contiguous() and frame.is_contiguous()
    m3 = (C.c_float * 3)(*[float(v) for v in mean])
    s3 = (C.c_float * 3)(*[float(v) for v in std])
    L.check(L.load().hm_crop_batch(L.ptr(frame), H, W, L.ptr(boxes_rec), L.ptr(out), B, P, m3, s3, L.current_stream()),
            "hm_crop_batch")
    return out


def crop_boxes_aa(boxes, P: int = 256) -> torch.Tensor:
    """boxes: iterable of (cx, cy, size, flip) -> ONE uint8 host tensor for the anti-aliased crop: the n hm_crop_aa_box records,
    then the n x 49 fp32 taps (one upload carries both).  Raises for a size whose blur exceeds sigma 12 (radius 48)."""
    lib = L.load()
    n = len(boxes)
    arr = (L.CropAaBox * n)()
    taps = (C.c_float * (n * L.HM_CROP_AA_TAPS))()
    for i, (cx, cy, size, flip) in enumerate(boxes):
        t = C.cast(C.byref(taps, i * L.HM_CROP_AA_TAPS * 4), C.POINTER(C.c_float))
        L.check(lib.hm_crop_aa_box_from_bbox(float(cx), float(cy), float(size), int(bool(flip)), P, C.byref(arr[i]), t),
                "hm_crop_aa_box_from_bbox")
    return torch.frombuffer(bytearray(bytes(arr) + bytes(taps)), dtype=torch.uint8).clone()


def crop_batch_aa(frame: torch.Tensor, rec: torch.Tensor, mean, std, P: int = 256, out: Optional[torch.Tensor] = None,
                  first: int = 0, count: Optional[int] = None) -> torch.Tensor:
    """hm_crop_batch_aa.  frame (H,W,3) uint8 BGR on device; rec: crop_boxes_aa's tensor on the device, n hands.  The launch
    serves hands [first, first + count) of it (default: all) -- the hands of one frame among several frames' records.
    ``out``: a contiguous (count,3,P,P) fp32 slice to fill."""
    _dev(frame, rec, out)
    H, W, _ = frame.shape
    rsz, tsz = C.sizeof(L.CropAaBox), 4 * L.HM_CROP_AA_TAPS
    n = rec.numel() // (rsz + tsz)
    B = n - first if count is None else count
    assert rec.dtype == torch.uint8 and rec.is_contiguous() and rec.numel() == n * (rsz + tsz) and 0 <= first and B > 0 and first + B <= n
    if out is None:
        out = torch.empty(B, 3, P, P, device=frame.device, dtype=torch.float32)
    assert out.shape == (B, 3, P, P) and out.dtype == torch.float32 and out.is_contiguous() and frame.is_contiguous()
    m3 = (C.c_float * 3)(*[float(v) for v in mean])
    s3 = (C.c_float * 3)(*[float(v) for v in std])
    base = rec.data_ptr()
    L.check(L.load().hm_crop_batch_aa(L.ptr(frame), H, W, base + first * rsz, base + n * rsz + first * tsz, L.ptr(out), B, P,
                                      m3, s3, L.current_stream()), "hm_crop_batch_aa")
    return out


def _chk(t: torch.Tensor, dtype, shape, what: str) -> None:
    if t.dtype != dtype or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise ValueError(f"{what}: expected a contiguous {dtype} tensor of shape {tuple(shape)}, got {t.dtype} {tuple(t.shape)}")


def det_match(pred: torch.Tensor, pred_count: torch.Tensor, labels: torch.Tensor, label_count: torch.Tensor,
              iouv: torch.Tensor):
    """hm_det_match.  pred (N, stride, 6) fp32 [xyxy, conf, cls], pred_count (N,) int32, labels (N, lmax, 5) fp32 [cls, xyxy],
    label_count (N,) int32, iouv (niou,) fp32, all contiguous device tensors -> correct (N, stride, niou) uint8,
    best_iou (N, stride) fp32, matched (N, stride) int32.  Asynchronous on the current stream."""
    _dev(pred, pred_count, labels, label_count, iouv)
    if pred.dim() != 3 or labels.dim() != 3:
        raise ValueError(f"det_match: pred {tuple(pred.shape)} / labels {tuple(labels.shape)}: expected (N, stride, 6) and (N, lmax, 5)")
    N, stride, lmax, niou = int(pred.shape[0]), int(pred.shape[1]), int(labels.shape[1]), int(iouv.numel())
    _chk(pred, torch.float32, (N, stride, 6), "det_match pred")
    _chk(labels, torch.float32, (N, lmax, 5), "det_match labels")
    _chk(pred_count, torch.int32, (N,), "det_match pred_count")
    _chk(label_count, torch.int32, (N,), "det_match label_count")
    _chk(iouv, torch.float32, (niou,), "det_match iouv")
    correct = torch.empty(N, stride, niou, dtype=torch.uint8, device=pred.device)
    best_iou = torch.empty(N, stride, dtype=torch.float32, device=pred.device)
    matched = torch.empty(N, stride, dtype=torch.int32, device=pred.device)
    L.check(L.load().hm_det_match(L.ptr(pred), L.ptr(pred_count), L.ptr(labels), L.ptr(label_count), L.ptr(iouv), N, stride,
                                  lmax, niou, L.ptr(correct), L.ptr(best_iou), L.ptr(matched), L.current_stream()), "hm_det_match")
    return correct, best_iou, matched


def det_ap(tp: torch.Tensor, conf: torch.Tensor, pred_cls: torch.Tensor, classes: torch.Tensor, n_labels: torch.Tensor,
           x101: torch.Tensor, px: torch.Tensor, v5_metric: bool = False):
    """hm_det_ap.  tp (P, niou) uint8, conf (P,) fp32, pred_cls (P,) fp32, ALREADY sorted by descending confidence;
    classes (nc,) fp32, n_labels (nc,) int32; x101 (101,) and px (1000,) fp64 -> ap (nc, niou), p (nc, 1000), r (nc, 1000)
    fp64.  Asynchronous on the current stream."""
    _dev(tp, conf, pred_cls, classes, n_labels, x101, px)
    if tp.dim() != 2:
        raise ValueError(f"det_ap: tp {tuple(tp.shape)}: expected (P, niou)")
    P, niou, nc = int(tp.shape[0]), int(tp.shape[1]), int(classes.numel())
    _chk(tp, torch.uint8, (P, niou), "det_ap tp")
    _chk(conf, torch.float32, (P,), "det_ap conf")
    _chk(pred_cls, torch.float32, (P,), "det_ap pred_cls")
    _chk(classes, torch.float32, (nc,), "det_ap classes")
    _chk(n_labels, torch.int32, (nc,), "det_ap n_labels")
    _chk(x101, torch.float64, (101,), "det_ap x101")
    _chk(px, torch.float64, (1000,), "det_ap px")
    lib = L.load()
    ap = torch.empty(nc, niou, dtype=torch.float64, device=tp.device)
    p = torch.empty(nc, 1000, dtype=torch.float64, device=tp.device)
    r = torch.empty(nc, 1000, dtype=torch.float64, device=tp.device)
    nbytes = int(lib.hm_det_ap_workspace_bytes(P, nc, niou))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=tp.device) if nbytes else None
    L.check(lib.hm_det_ap(L.ptr(tp) if P else None, L.ptr(conf) if P else None, L.ptr(pred_cls) if P else None, P,
                          L.ptr(classes), L.ptr(n_labels), nc, niou, L.ptr(x101), L.ptr(px), int(bool(v5_metric)), L.ptr(ap),
                          L.ptr(p), L.ptr(r), L.ptr(ws), nbytes, L.current_stream()), "hm_det_ap")
    return ap, p, r


def det_ap_curve(recall: torch.Tensor, precision: torch.Tensor, x101: torch.Tensor, v5_metric: bool = False):
    """hm_det_ap_curve.  recall, precision (n,) fp64 device tensors -> ap (1,), mpre (n + 2,), mrec (n + 2,) fp64."""
    _dev(recall, precision, x101)
    n = int(recall.numel())
    _chk(recall, torch.float64, (n,), "det_ap_curve recall")
    _chk(precision, torch.float64, (n,), "det_ap_curve precision")
    _chk(x101, torch.float64, (101,), "det_ap_curve x101")
    ap = torch.empty(1, dtype=torch.float64, device=recall.device)
    mpre = torch.empty(n + 2, dtype=torch.float64, device=recall.device)
    mrec = torch.empty(n + 2, dtype=torch.float64, device=recall.device)
    L.check(L.load().hm_det_ap_curve(L.ptr(recall), L.ptr(precision), n, L.ptr(x101), int(bool(v5_metric)), L.ptr(ap),
                                     L.ptr(mpre), L.ptr(mrec), L.current_stream()), "hm_det_ap_curve")
    return ap, mpre, mrec


# ----------------------------------------------------------------------------- detector test-time augmentation (csrc/tta.hip)
_DT_TTA = {torch.bfloat16: L.HM_DTYPE_BF16, torch.float16: L.HM_DTYPE_F16, torch.float32: L.HM_DTYPE_F32}


def tta_sizes(h: int, w: int, ratio: float, gs: int = 32):
    """hm_tta_sizes: scale_img's (resized h, resized w, padded h, padded w) for an h x w network input."""
    sz = (C.c_int * 4)()
    L.check(L.load().hm_tta_sizes(int(h), int(w), float(ratio), int(gs), sz), "hm_tta_sizes")
    return tuple(sz)


def tta_tables(h: int, w: int, ratio: float, gs: int = 32, flip_lr: bool = False) -> torch.Tensor:
    """hm_tta_tables: the tap table of one scale as an int32 host tensor of 4 * wp + 4 * hp entries (tap0 | tap1 | weight0 |
    weight1 for the columns, then for the rows; the weights are fp32 bits)."""
    _, _, hp, wp = tta_sizes(h, w, ratio, gs)
    tab = (C.c_int32 * (4 * wp + 4 * hp))()
    L.check(L.load().hm_tta_tables(int(h), int(w), float(ratio), int(gs), int(bool(flip_lr)), tab), "hm_tta_tables")
    return torch.frombuffer(bytearray(bytes(tab)), dtype=torch.int32).clone()


def tta_scale(x: torch.Tensor, ratio: float, gs: int = 32, flip_lr: bool = False, tab: Optional[torch.Tensor] = None) -> torch.Tensor:
    """hm_tta_scale.  x (nb, h, w, 8) fp16 / bf16 / fp32 on the device, channels 0-2 the image -> (nb, hp, wp, 8): mirrored
    when ``flip_lr``, resized by ``ratio`` and padded with 0.447 to multiples of ``gs``.  ``tab``: tta_tables' tensor on the
    device (built and uploaded here when None)."""
    _dev(x, tab)
    if x.dim() != 4 or x.shape[3] != 8 or x.dtype not in _DT_TTA or not x.is_contiguous():
        raise ValueError(f"tta_scale: expected a contiguous (nb, h, w, 8) fp16 / bf16 / fp32 tensor, got {x.dtype} {tuple(x.shape)}")
    nb, h, w, _ = x.shape
    _, _, hp, wp = tta_sizes(h, w, ratio, gs)
    if tab is None:
        tab = tta_tables(h, w, ratio, gs, flip_lr).to(x.device)
    _chk(tab, torch.int32, (4 * wp + 4 * hp,), "tta_scale: tab")
    y = torch.empty(nb, hp, wp, 8, dtype=x.dtype, device=x.device)
    L.check(L.load().hm_tta_scale(L.ptr(x), L.ptr(y), L.ptr(tab), nb, h, w, float(ratio), int(gs), _DT_TTA[x.dtype], L.current_stream()),
            "hm_tta_scale")
    return y


def yolo_decode_batch_tta(raw: torch.Tensor, pred: torch.Tensor, row0: int, ny: int, nx: int, nc: int, stride: float, anchors6,
                          nb: int, pred_rows_per_image: int, scale: float, flip_lr: bool, full_w: float) -> None:
    """hm_yolo_decode_batch_tta: raw (nb * ny * nx, 3 * (5 + nc)) fp32 of one level -> rows [row0, row0 + 3 * ny * nx) of every
    image's ``pred_rows_per_image`` rows of pred (.., 5 + nc) fp32, xywh divided by ``scale`` and x mirrored in ``full_w``
    when ``flip_lr``."""
    _dev(raw, pred)
    no = 5 + nc
    _chk(raw, torch.float32, (nb * ny * nx, 3 * no), "yolo_decode_batch_tta: raw")
    if pred.dtype != torch.float32 or not pred.is_contiguous() or pred.shape[-1] != no or row0 < 0 or \
            row0 + 3 * ny * nx > pred_rows_per_image or pred.numel() < nb * pred_rows_per_image * no:
        raise ValueError("yolo_decode_batch_tta: pred must be contiguous fp32 (.., 5 + nc) with nb * pred_rows_per_image rows, "
                         "the level's rows inside an image's")
    anc = (C.c_float * 6)(*[float(v) for v in anchors6])
    L.check(L.load().hm_yolo_decode_batch_tta(L.ptr(raw), 3 * no, L.ptr(pred), int(row0), ny, nx, nc, float(stride), anc, nb,
                                              int(pred_rows_per_image), float(scale), int(bool(flip_lr)), float(full_w),
                                              L.current_stream()), "hm_yolo_decode_batch_tta")
