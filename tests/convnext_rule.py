"""The ConvNeXt-base SAR backbone (rootnet/convnext.py:15-50 Block, :66-114 ConvNeXt.forward, :127-151 LayerNorm) restated in
torch from the state dict: the CPU rule of tests/test_gpu_convnext.py, runnable in fp32 and fp64.  The committed fixture
tests/golden/convnext_base.npz (written by the reference's own module, tools/gen_golden_convnext.py) pins it
(tests/test_convnext_host.py).

emu='f16' / 'bf16' is the same function with the roundings of the HIP route put where its kernels have them: the GEMM
weights (the layer scale folded into pwconv2 first, in fp32), the stem's patches, every LayerNorm output that feeds a GEMM,
the GELU output and the final map are rounded to the 16-bit type; everything else (the residual stream, the depthwise
convolution, the statistics, the accumulations) keeps ``dtype``.  Against it the GPU differs by summation order and by
values that round the other way at a tie."""
import torch
import torch.nn.functional as F

DEPTHS = (3, 3, 27, 3)
DIMS = (128, 256, 512, 1024)
EPS = 1e-6
PREFIX = "backbone."


def patches(seed, n=1, size=256):
    """The seeded input patches of the fixture and of the GPU tests: (n, 3, size, size) fp32, a smooth signed image plus
    noise, about unit variance (the range of the normalised crops)."""
    g = torch.Generator().manual_seed(1000 + seed)
    coarse = torch.randn(n, 3, size // 16 + 1, size // 16 + 1, generator=g)
    smooth = F.interpolate(coarse, size=(size, size), mode="bilinear", align_corners=True)
    return (smooth + 0.3 * torch.randn(n, 3, size, size, generator=g)).float().contiguous()


def _ln(x, w, b):
    """LayerNorm over the LAST dim (channels_first in the reference is the same per-pixel statistic, biased variance)."""
    u = x.mean(-1, keepdim=True)
    s = (x - u).pow(2).mean(-1, keepdim=True)
    return (x - u) / torch.sqrt(s + EPS) * w + b


def block(sd, pre, x, q=lambda t: t, fold=False):
    """Block.forward on an NHWC stream x (B, H, W, C).  fold: gamma folded into pwconv2 before q (the engine's weights)."""
    c = x.shape[-1]
    y = F.conv2d(x.permute(0, 3, 1, 2), sd[pre + "dwconv.weight"], sd[pre + "dwconv.bias"], padding=3, groups=c).permute(0, 2, 3, 1)
    y = q(_ln(y, sd[pre + "norm.weight"], sd[pre + "norm.bias"]))
    y = q(F.gelu(F.linear(y, q(sd[pre + "pwconv1.weight"]), sd[pre + "pwconv1.bias"])))
    g = sd[pre + "gamma"]
    if fold:
        return x + F.linear(y, q(folded_pwconv2(sd, pre)[0]), g * sd[pre + "pwconv2.bias"])
    return x + g * F.linear(y, q(sd[pre + "pwconv2.weight"]), sd[pre + "pwconv2.bias"])


def folded_pwconv2(sd, pre):
    """(gamma[:, None] * W2, gamma * b2): x + gamma * (W2 h + b2) = x + (gamma W2) h + gamma b2."""
    g = sd[pre + "gamma"]
    return g[:, None] * sd[pre + "pwconv2.weight"], g * sd[pre + "pwconv2.bias"]


@torch.no_grad()
def forward(sd, img, dtype=torch.float64, emu=None, taps=False, prefix=PREFIX):
    """ConvNeXt.forward: img (B, 3, 256, 256) -> the post-norm map (B, 8, 8, 1024) NHWC in ``dtype`` (the reference returns
    its NCHW permutation).  taps=True also returns the NHWC stream after the stem and after each of the four stages."""
    if emu is None:
        q = lambda t: t                                                             # noqa: E731
    else:
        lo = {"f16": torch.float16, "bf16": torch.bfloat16}[emu]
        q = lambda t: t.to(lo).to(dtype)                                            # noqa: E731
    fold = emu is not None
    sd = {k[len(prefix):]: v.to(dtype) for k, v in sd.items() if k.startswith(prefix) and not k.startswith(prefix + "head.")}
    d = "downsample_layers."
    x = F.conv2d(q(img.to(dtype)), q(sd[d + "0.0.weight"]), sd[d + "0.0.bias"], stride=4).permute(0, 2, 3, 1)
    x = _ln(x, sd[d + "0.1.weight"], sd[d + "0.1.bias"])
    seen = [x]
    for i in range(4):
        if i > 0:
            y = q(_ln(x, sd[d + f"{i}.0.weight"], sd[d + f"{i}.0.bias"]))
            x = F.conv2d(y.permute(0, 3, 1, 2), q(sd[d + f"{i}.1.weight"]), sd[d + f"{i}.1.bias"], stride=2).permute(0, 2, 3, 1)
        for j in range(DEPTHS[i]):
            x = block(sd, f"stages.{i}.{j}.", x, q, fold)
        seen.append(x)
    out = q(_ln(x, sd["norm.weight"], sd["norm.bias"])).contiguous()
    return (out, seen) if taps else out


def tap_sample(seen):
    """The strided sample of the streams the fixture stores: every 8th pixel of the 64-wide map down to every pixel of the
    8-wide one (8 x 8 positions each), every 8th channel."""
    return [s[:, ::max(1, s.shape[1] // 8), ::max(1, s.shape[2] // 8), ::8].contiguous() for s in seen]


@torch.no_grad()
def root_depth(root_sd, feat, k_value):
    """ResRootNet.forward_coord (rootnet/Model_RGB.py:262-287) on the NHWC map: GAP, the 1 x 1 depth layer, times k."""
    dt = feat.dtype
    gap = feat.reshape(feat.shape[0], -1, feat.shape[-1]).mean(1)
    g = gap @ root_sd["depth_layer.weight"].to(dt).reshape(-1) + root_sd["depth_layer.bias"].to(dt).reshape(-1)[0]
    return g * torch.as_tensor(k_value, dtype=dt).reshape(-1)
