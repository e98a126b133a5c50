"""Operands of the exact-integer GEMM / convolution tests, the shapes those tests run, and the comparison they end in.

The strict kernel tests feed small integers, so that every product and every partial sum is an integer below 2^24 and hence
exact in fp32 whatever the summation order, and then demand torch.equal.  That pins tile, ring and lane maps only if the DATA
tells one operand index from another: an operand that is constant (or periodic with the tile width) along an axis lets a
kernel that reads the wrong element along that axis pass.  So every operand here is a hash of the flat element index
(synth._hash_u32, seeded by synth.name_seed of a tag): each element depends on all of its indices, with no period.
tests/test_exact_data_host.py applies a catalogue of index faults to the operands of the torch reference, at every shape
listed below, and requires each fault to change more than half of the outputs.

Plain helper module (imported like sar_rule.py); torch-CPU only, nothing here touches the compiled library.
"""
import torch

from hamer_yolo_amd import synth

EXACT_LIMIT = float(1 << 24)      # integers of magnitude below 2^24 are exact in fp32, and so is every sum that stays below it


def ints(tag, shape, lo, hi, seed=0, chunk=1 << 24):
    """fp32 tensor of integers in [lo, hi]: element i (flat, row-major) is lo + hash(i; tag, seed) % (hi - lo + 1)."""
    assert hi >= lo
    n = 1
    for s in shape:
        n *= int(s)
    out = torch.empty(n, dtype=torch.float32)
    ns = synth.name_seed(tag, seed)
    for start in range(0, n, chunk):
        stop = min(n, start + chunk)
        h = synth._hash_u32(torch.arange(start, stop, dtype=torch.int64), ns)
        out[start:stop] = (h % (hi - lo + 1) + lo).to(torch.float32)
    return out.reshape(*shape)


def _amax(t):
    return 0.0 if t is None else float(t.abs().max())


def exact_bound(x, w, K, bias=None, resid=None, scale=1.0, unit=1.0):
    """Largest magnitude any partial or final sum can reach, in units of the smallest step: max|x| max|w| K + max|bias| +
    max|resid|, measured on the data (scale: product of the largest operand scales, unit: of the smallest; 1 without scales)."""
    return (_amax(x) * _amax(w) * K * scale + _amax(bias) + _amax(resid)) / unit


def _shape_seed(*dims):
    s = 0
    for d in dims:
        s = (s * 1000003 + int(d)) & 0x7FFFFFFF
    return s


# ------------------------------------------------------------------------------------------------ builders
def gemm_case(M, N, K, bias=True, resid=None, resid_rows=None):
    """x (M,K) in -3..3, w (N,K) in -2..2, bias (N,) in -4..4 or None, resid (resid_rows or M, N) in -resid..resid or None
    (the tests use 5 and 510), all fp32 integers; asserts the exactness bound on what it built."""
    sd = _shape_seed(M, N, K)
    x = ints("exact.gemm.x", (M, K), -3, 3, sd)
    w = ints("exact.gemm.w", (N, K), -2, 2, sd)
    b = ints("exact.gemm.bias", (N,), -4, 4, sd) if bias else None
    r = ints("exact.gemm.resid", (resid_rows or M, N), -int(resid), int(resid), sd) if resid else None
    bound = exact_bound(x, w, K, b, r)
    assert bound < EXACT_LIMIT, (M, N, K, bound)
    return x, w, b, r


def conv_case(n, Ci, Co, k, H, W):
    """x (n,Ci,H,W) in -2..2, w (Co,Ci,k,k) in -1..1, bias (Co,) in -3..3.  The seed leaves n out, so the first images of a
    large batch are the whole of a small one (the host test convolves two images of the 140-frame cases)."""
    sd = _shape_seed(Ci, Co, k, H, W)
    x = ints("exact.conv.x", (n, Ci, H, W), -2, 2, sd)
    w = ints("exact.conv.w", (Co, Ci, k, k), -1, 1, sd)
    b = ints("exact.conv.bias", (Co,), -3, 3, sd)
    bound = exact_bound(x, w, Ci * k * k, b)
    assert bound < EXACT_LIMIT, (n, Ci, Co, k, H, W, bound)
    return x, w, b


def fp8_case(M, N, K):
    """MXFP8 operands whose every product and sum is exact: xi (M,K) in -4..4 and wi (N,K) in -3..3 (integers that e4m3
    holds exactly), E8M0 block scales xs (K/32, M) of 2^-1..2^2 and per-row weight scales ws (N,) of 2^-1..2^1.
    Returns x8, xs, w8, ws (the bytes and scales the kernel takes) and xi, wi (the same values as fp32)."""
    sd = _shape_seed(M, N, K)
    xi = ints("exact.fp8.x", (M, K), -4, 4, sd)
    wi = ints("exact.fp8.w", (N, K), -3, 3, sd)
    xs = (127 + ints("exact.fp8.xs", (K // 32, M), -1, 2, sd)).to(torch.uint8)
    ws = torch.ldexp(torch.ones(N), ints("exact.fp8.ws", (N,), -1, 1, sd).to(torch.int32))
    x8 = xi.to(torch.float8_e4m3fn)
    w8 = wi.to(torch.float8_e4m3fn)
    assert torch.equal(x8.float(), xi) and torch.equal(w8.float(), wi)            # e4m3-exact
    sx = torch.ldexp(torch.ones(()), xs.to(torch.int32) - 127)
    bound = exact_bound(xi, wi, K, scale=float(sx.max()) * float(ws.max()), unit=float(sx.min()) * float(ws.min()))
    assert bound < EXACT_LIMIT, (M, N, K, bound)
    return x8.view(torch.uint8), xs, w8.view(torch.uint8), ws, xi, wi


def fp8_reference(xi, xs, wi, ws):
    """fp64 statement of the scaled product: (xi * 2^(xs - 127) per 32-wide K block) @ (wi * ws per row)^T."""
    sx = torch.ldexp(torch.ones((), dtype=torch.float64), xs.to(torch.int32) - 127)        # (K/32, M)
    xd = xi.double() * sx.t().repeat_interleave(32, dim=1)
    return xd @ (wi.double() * ws.double()[:, None]).t()


# ------------------------------------------------------------------------------------------------ the shapes of the GPU tests
# hm_gemm, (M, N, K)
GEMM_ASYMMETRIC = [(192, 256, 128)]
GEMM_TILE_VARIANTS = [(300, 260, 64), (513, 388, 128), (1000, 1284, 448), (700, 516, 192), (257, 260, 1280)]
GEMM_TILE_RULE_HANDS = [16, 17, 23, 40, 45, 68, 72]                      # M = hands * 192
GEMM_TILE_RULE_NK = [(3840, 128, "store"), (1280, 192, "resid"), (5120, 128, "store")]
GEMM_DEEP_PREFETCH = [(300, 260, 64), (513, 388, 128), (1000, 1284, 192), (700, 516, 448), (257, 260, 1280), (1536, 512, 5120)]
GEMM_PERSISTENT = [(2048, 256, 128), (2304, 2560, 128), (4096, 4096, 192), (2560, 10240, 128), (12288, 3840, 1280), (5120, 5120, 64 * 7)]
GEMM_PERSISTENT_FALLBACK = [(300, 260, 64), (2048, 2048, 64), (1000, 1284, 192)]
GEMM_INLOOP_RESIDUAL = [(512, 1280, 1280), (768, 256, 1344), (256, 512, 5120), (2304, 1280, 1280)]
GEMM_INLOOP_RESIDUAL_RANGE = 510
# leading dimensions wider than the row: one shape of whole 256 x 256 tiles that the persistent kernel (>= 8 tiles, K >= 128)
# and the in-loop residual kernel (K >= 1280) both take, and one ragged in M and N
GEMM_STRIDED = [(512, 1280, 1280), (300, 260, 128)]
# hm_gemm_f32: the six ViT-H (K, N) of the precise route at one and seven hands, and M = 1 with an N that fills no tile
GEMM_F32_KN = [(768, 1280), (1280, 3840), (1280, 1280), (1280, 5120), (5120, 1280), (1280, 6 * 1024)]
GEMM_F32_HANDS = [1, 7]
GEMM_F32_RAGGED = [(1, 1280 - 32, 768), (1, 3840 - 32, 1280)]
GEMM_F32_STRIDED = [(192, 1280, 1280), (77, 100, 96)]
# hm_gemm_fp8
GEMM_FP8 = [(272, 320, 384)]
# hm_conv2d_nhwc, (n, Ci, Co, k, stride, H, W)
CONV_BASIC = [(2, 16, 32, 3, 1, 9, 11)]
CONV_EVERY_TILE = [(2, 16, 32, 3, 1, 9, 11), (2, 32, 264, 3, 2, 21, 19), (2, 64, 72, 1, 1, 33, 35), (2, 8, 256, 3, 1, 30, 34)]
CONV_K_GROUPS = [(2, 128, 72, 3, 1, 12, 20), (2, 128, 264, 3, 2, 47, 79), (2, 512, 40, 1, 1, 24, 40), (2, 512, 64, 3, 1, 12, 20)]
CONV_K_GROUPS_SPLIT = [False, False, False, True]                         # the last one runs on split-K scratch
CONV_LEAN_LOADER = [(3, 64, 64, 3, 1, 23, 37), (3, 128, 72, 3, 2, 47, 79), (3, 256, 128, 1, 1, 24, 40), (3, 128, 96, 5, 1, 13, 13),
                    (3, 512, 264, 3, 1, 12, 20), (3, 64, 40, 3, 2, 9, 11)]
CONV_SERIAL_K = [(40, 1024, 512, 1, 1, 12, 20), (72, 256, 256, 3, 1, 12, 20), (48, 512, 264, 3, 1, 12, 20), (36, 256, 128, 3, 1, 24, 40),
                 (140, 512, 64, 3, 2, 24, 40)]
CONV_SPLIT_K = [(2, 256, 256, 3, 1, 12, 20)]
CONV_F32 = [(2, 16, 32, 3, 1, 9, 11), (2, 64, 72, 3, 2, 9, 11), (2, 256, 128, 1, 1, 9, 11)]


def gemm_tile_rule_shapes():
    return [(h * 192, N, K, epi) for h in GEMM_TILE_RULE_HANDS for (N, K, epi) in GEMM_TILE_RULE_NK]


def gemm_f32_shapes():
    return [(h * 192, N, K) for h in GEMM_F32_HANDS for (K, N) in GEMM_F32_KN] + GEMM_F32_RAGGED


# ------------------------------------------------------------------------------------------------ the comparison
def _blocks(idx, n):
    b = sorted(set((idx // 64).tolist()))
    head = ", ".join(str(v) for v in b[:24]) + (", ..." if len(b) > 24 else "")
    return f"{len(b)} of {(n + 63) // 64}: [{head}]"


def mismatch_report(got, ref, what=""):
    """None when got equals ref element for element, else a description of the difference: the count of wrong elements, the
    first wrong (row, col) with both values, and the 64-row / 64-column blocks that hold errors (a tile or ring fault shows
    as a pattern of blocks).  4-D (n, C, H, W) results are read as the implicit GEMM sees them: rows = pixels, cols = channels."""
    got, ref = got.detach().cpu(), ref.detach().cpu()
    if got.shape != ref.shape:
        return f"{what}: shape {tuple(got.shape)} != expected {tuple(ref.shape)}"
    if got.dtype != ref.dtype:
        return f"{what}: dtype {got.dtype} != expected {ref.dtype}"
    if torch.equal(got, ref):
        return None
    if got.dim() == 4:
        got, ref = (t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]) for t in (got, ref))
    got2, ref2 = got.reshape(-1, got.shape[-1]), ref.reshape(-1, ref.shape[-1])
    bad = got2 != ref2
    if got2.is_floating_point():
        bad &= ~(got2.isnan() & ref2.isnan())
    rows, cols = bad.nonzero(as_tuple=True)
    if rows.numel() == 0:                           # torch.equal is False for NaN == NaN only
        return f"{what}: NaN in matching positions of got and expected ({int(got2.isnan().sum())} elements)"
    r0, c0 = int(rows[0]), int(cols[0])
    M, N = got2.shape
    return (f"{what}: {rows.numel()} of {M * N} elements wrong; first at (row {r0}, col {c0}): got {got2[r0, c0].item()!r}, "
            f"expected {ref2[r0, c0].item()!r}; 64-row blocks with errors {_blocks(rows, M)}; "
            f"64-column blocks with errors {_blocks(cols, N)}")


def assert_exact(got, ref, what=""):
    """assert torch.equal(got, ref), with a message that locates the fault."""
    msg = mismatch_report(got, ref, str(what))
    assert msg is None, msg
