"""ConvNextEngine: the ConvNeXt-base SAR backbone (rootnet/convnext.py) + ResRootNet's depth layer on libhamer_hip, with the
interface of RootNetEngine (features / forward / depth_of), so EstimateRGB picks one of the two and forks nowhere else.

The residual stream is fp32 NHWC.  Per block: hm_dwconv7_ln (depthwise 7 x 7 + LayerNorm -> 16-bit), hm_gemm HM_EPI_GELU
(C -> 4C, 16-bit), hm_gemm HM_EPI_RESID_F32 (4C -> C, added to the stream in place).  Downsample layers: hm_ln_patchify2 +
hm_gemm HM_EPI_F32; the stem: hm_stem4_im2col + hm_gemm HM_EPI_F32 + hm_layernorm.  The final LayerNorm writes the 16-bit
(B, 8, 8, 1024) map the SAR head and hm_gap_linear read.

Load-time work (host_weights): the layer scale ``gamma`` is folded into pwconv2's rows and bias in fp32 before the weights are
rounded, the depthwise weight is transposed to tap-major [49][C], the 2 x 2 downsample weights are permuted to the (ky, kx, c)
order of hm_ln_patchify2, the stem weight is padded from K = 48 to 64.  ``backbone.head.*`` (the unused 21841-class
classifier) is neither read nor uploaded."""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional

import torch

from .. import lib as L
from . import convnext_arch as arch

_W16 = ("stem.w", "down.w", "w1", "w2")          # name endings of the GEMM weights: stored in the 16-bit operand type


def host_weights(net_sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """The engine's operands on the host, all fp32 (the GEMM weights are rounded on upload), named by what the kernels take."""
    missing = [k for k in arch.key_shapes() if k not in net_sd]
    if missing:
        raise KeyError(f"ConvNeXt backbone weights missing from the checkpoint: {missing[:4]}{' ...' if len(missing) > 4 else ''}")
    shapes = arch.key_shapes()

    def f(k):                                               # every key is read here, once
        t = net_sd[k]
        if tuple(t.shape) != shapes[k]:
            raise ValueError(f"{k}: shape {tuple(t.shape)}, ConvNeXt-base has {shapes[k]}")
        return t.detach().float().cpu()
    d = arch.PREFIX + "downsample_layers."
    w: Dict[str, torch.Tensor] = {}
    stem = torch.zeros(arch.DIMS[0], 64)
    stem[:, :48] = f(d + "0.0.weight").reshape(arch.DIMS[0], 48)          # (c, ky, kx): hm_stem4_im2col's order
    w["stem.w"], w["stem.b"] = stem, f(d + "0.0.bias")
    w["stem.ln_g"], w["stem.ln_b"] = f(d + "0.1.weight"), f(d + "0.1.bias")
    for i in range(1, 4):
        w[f"{i}.ln_g"], w[f"{i}.ln_b"] = f(d + f"{i}.0.weight"), f(d + f"{i}.0.bias")
        w[f"{i}.down.w"] = f(d + f"{i}.1.weight").permute(0, 2, 3, 1).reshape(arch.DIMS[i], 4 * arch.DIMS[i - 1]).contiguous()
        w[f"{i}.down.b"] = f(d + f"{i}.1.bias")
    for n, (pre, _, c) in enumerate(arch.blocks()):
        g = f(pre + "gamma")
        w[f"b{n}.dw_w"] = f(pre + "dwconv.weight").reshape(c, 49).t().contiguous()          # [49][C]
        w[f"b{n}.dw_b"] = f(pre + "dwconv.bias")
        w[f"b{n}.ln_g"], w[f"b{n}.ln_b"] = f(pre + "norm.weight"), f(pre + "norm.bias")
        w[f"b{n}.w1"], w[f"b{n}.b1"] = f(pre + "pwconv1.weight").contiguous(), f(pre + "pwconv1.bias")
        w[f"b{n}.w2"] = (g[:, None] * f(pre + "pwconv2.weight")).contiguous()               # x + gamma * (W h + b)
        w[f"b{n}.b2"] = g * f(pre + "pwconv2.bias")
    w["norm.g"], w["norm.b"] = f(arch.PREFIX + "norm.weight"), f(arch.PREFIX + "norm.bias")
    return w


class ConvNextEngine:
    def __init__(self, net_sd: Dict[str, torch.Tensor], root_sd: Optional[Dict[str, torch.Tensor]], device="cuda", dtype=torch.float16):
        if dtype not in (torch.float16, torch.bfloat16):
            raise ValueError("ConvNextEngine: the fp32 route of the ConvNeXt backbone does not exist yet (dtype float16 or bfloat16)")
        if not torch.cuda.is_available():
            raise L.HipLibraryError("ConvNextEngine needs an MI355X (HIP device); there is no CPU fallback")
        self.lib = L.load()
        self.device, self.dtype = torch.device(device), dtype
        self.precise = False
        self.dt = L.HM_DTYPE_BF16 if dtype == torch.bfloat16 else L.HM_DTYPE_F16
        self.w = {k: v.to(self.device, dtype if k.endswith(_W16) else torch.float32).contiguous() for k, v in host_weights(net_sd).items()}
        self.depth_w, self.depth_b = None, 0.0          # a checkpoint without ``rootnet``: features only (the SAR head's)
        if root_sd is not None:
            self.depth_w = root_sd["depth_layer.weight"].reshape(-1).to(self.device, torch.float32).contiguous()
            if self.depth_w.numel() != arch.DIMS[3]:
                raise ValueError(f"rootnet depth_layer has {self.depth_w.numel()} input channels, ConvNeXt-base features have {arch.DIMS[3]}")
            self.depth_b = float(root_sd["depth_layer.bias"].reshape(-1)[0])
        self._ws: Dict[int, Dict[str, torch.Tensor]] = {}

    def weight_bytes(self) -> int:
        """Device bytes of every operand the engine holds (tests: the classifier is not among them)."""
        n = sum(v.numel() * v.element_size() for v in self.w.values())
        return n + (self.depth_w.numel() * 4 if self.depth_w is not None else 0)

    def _workspace(self, B: int, P: int) -> Dict[str, torch.Tensor]:
        ws = self._ws.get((B, P))
        if ws is None:
            e = dict(device=self.device)
            s = P // 4
            px = B * s * s
            ws = {"t": torch.empty(px * arch.DIMS[0], dtype=self.dtype, **e),              # LayerNorm / patchify output (X of a GEMM)
                  "h": torch.empty(px * 4 * arch.DIMS[0], dtype=self.dtype, **e)}          # GELU output; the stem's patches
            for i, c in enumerate(arch.DIMS):
                ws[f"x{i}"] = torch.empty(B, s >> i, s >> i, c, dtype=torch.float32, **e)  # the fp32 residual stream of stage i
            self._ws = {(B, P): ws}                                                        # keep one batch size's buffers
        return ws

    def _gemm(self, x, w, out, bias, M, N, K, epi, resid=None):
        a = L.GemmArgs(L.ptr(x), L.ptr(w), L.ptr(out), L.ptr(bias), L.ptr(resid), M, N, K, K, K, N, N if resid is not None else 0, 0,
                       epi, self.dt)
        L.check(self.lib.hm_gemm(C.byref(a), L.current_stream()), "hm_gemm")

    def features(self, img: torch.Tensor) -> torch.Tensor:
        """img (B, 3, P, P) fp32 normalised RGB planes (the layout hm_crop_batch writes; P = 256, any multiple of 32) ->
        (B, P/32, P/32, 1024) NHWC in the engine's 16-bit dtype: ConvNeXt.forward's post-norm map (convnext.py:108-114)."""
        B, ch, H, Wd = img.shape
        assert ch == 3 and H == Wd and H % 32 == 0 and img.dtype == torch.float32
        img = img.contiguous()
        ws, w, s, lib, dt = self._workspace(B, H), self.w, L.current_stream(), self.lib, self.dt
        t, h = ws["t"], ws["h"]
        hw = H // 4
        L.check(lib.hm_stem4_im2col(L.ptr(img), L.ptr(h), B, H, Wd, dt, s), "hm_stem4_im2col")
        x = ws["x0"]
        c0 = arch.DIMS[0]
        # the stem's pre-LayerNorm fp32 output lives behind the patches in ``h``: px * 128 B of patches, px * 512 B of fp32,
        # px * 1024 B in all
        pre = h[B * hw * hw * 64:].view(torch.float32)[:B * hw * hw * c0]
        self._gemm(h, w["stem.w"], pre, w["stem.b"], B * hw * hw, c0, 64, L.HM_EPI_F32)
        L.check(lib.hm_layernorm(L.ptr(pre), L.ptr(w["stem.ln_g"]), L.ptr(w["stem.ln_b"]), L.ptr(x), L.HM_OUT_F32, B * hw * hw, c0,
                                 arch.LN_EPS, s), "hm_layernorm")
        n = 0
        for i, c in enumerate(arch.DIMS):
            if i > 0:
                cp = arch.DIMS[i - 1]
                L.check(lib.hm_ln_patchify2(L.ptr(x), L.ptr(w[f"{i}.ln_g"]), L.ptr(w[f"{i}.ln_b"]), L.ptr(t), B, hw, hw, cp,
                                            arch.LN_EPS, dt, s), "hm_ln_patchify2")
                hw //= 2
                x = ws[f"x{i}"]
                self._gemm(t, w[f"{i}.down.w"], x, w[f"{i}.down.b"], B * hw * hw, c, 4 * cp, L.HM_EPI_F32)
            M = B * hw * hw
            for _ in range(arch.DEPTHS[i]):
                p = f"b{n}."
                L.check(lib.hm_dwconv7_ln(L.ptr(x), L.ptr(w[p + "dw_w"]), L.ptr(w[p + "dw_b"]), L.ptr(w[p + "ln_g"]),
                                          L.ptr(w[p + "ln_b"]), L.ptr(t), B, hw, hw, c, arch.LN_EPS, dt, s), "hm_dwconv7_ln")
                self._gemm(t, w[p + "w1"], h, w[p + "b1"], M, 4 * c, c, L.HM_EPI_GELU)
                self._gemm(h, w[p + "w2"], x, w[p + "b2"], M, c, 4 * c, L.HM_EPI_RESID_F32, resid=x)
                n += 1
        out = torch.empty(B, hw, hw, arch.DIMS[3], device=self.device, dtype=self.dtype)
        L.check(lib.hm_layernorm(L.ptr(x), L.ptr(w["norm.g"]), L.ptr(w["norm.b"]), L.ptr(out), dt, B * hw * hw, arch.DIMS[3],
                                 arch.LN_EPS, s), "hm_layernorm")
        return out

    def forward(self, img: torch.Tensor, k_value: torch.Tensor) -> torch.Tensor:
        """depth (B,) = (GAP(features) . w + b) * k_value (ResRootNet.forward_coord on the hooked backbone output,
        Model_RGB.py:262-287, :335-337)."""
        kv = k_value.to(self.device, torch.float32).contiguous()      # (a pageable upload waits for the stream: before the backbone is queued)
        return self.depth_of(self.features(img), kv)

    def depth_of(self, f: torch.Tensor, kv: torch.Tensor) -> torch.Tensor:
        """ResRootNet.forward_coord on features already computed: f (B, 8, 8, 1024), kv (B,) fp32 on the device -> (B,)."""
        if self.depth_w is None:
            raise RuntimeError("RootNet is not loaded in the checkpoint!")
        B, h, w, c = f.shape
        assert c == arch.DIMS[3] and f.dtype == self.dtype and f.is_contiguous()
        depth = torch.empty(B, device=self.device, dtype=torch.float32)
        L.check(self.lib.hm_gap_linear(L.ptr(f), h * w, c, L.ptr(self.depth_w), self.depth_b, L.ptr(kv), L.ptr(depth), B, self.dt,
                                       L.current_stream()), "hm_gap_linear")
        return depth
