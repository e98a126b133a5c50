"""Operands of the exact-integer GEMM / convolution tests, the shapes those tests run, and the comparison they end in.

The strict kernel tests feed small integers, so that every product and every partial sum is an integer below 2^24 and hence
exact in fp32 whatever the summation order, and then demand torch.equal.  That pins tile, ring and lane maps only if the DATA
tells one operand index from another: an operand that is constant (or periodic with the tile width) along an axis lets a
kernel that reads the wrong element along that axis pass.  So every operand here is a hash of the flat element index
(synth._hash_u32, seeded by synth.name_seed of a tag): each element depends on all of its indices, with no period.
tests/test_exact_data_host.py applies a catalogue of index faults to the operands of the torch reference, at every shape
listed below, and requires each fault to change more than half of the outputs.

The LayerNorm kernels get the same treatment with other data (section "LayerNorm" below): rows whose mean is a small integer,
whose centred values are +-0.5 and whose rstd is exactly 1, so that y = sigma * gamma / 2 + beta is exact in fp32, bf16 and fp16
and the MXFP8 bytes and scales are those of the oracle quantiser; and a set of hostile rows with a per-row error bound for the
accuracy test.

The SAR hand-mesh head (section "SAR hand-mesh head") takes the GEMM integers through its seven GEMM entry points, with the
bound of an fp16 output added (|acc + bias| <= 2048), and has data of its own for the soft-argmax (few-hot logits whose softmax
is exactly 1 / m on a hashed support) and the post-processing (dyadic coordinates, transforms, roots and depth maps).

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


# ------------------------------------------------------------------------------------------------ LayerNorm
# Rows whose LayerNorm is exact in fp32 whatever the order of the two reductions.  x[r, c] = m_r + sigma(r, c) / 2 with a small
# hashed integer m_r and a hashed sign sigma whose second half-row is the negation of the first: every partial sum of the row is
# a small multiple of 0.5, the row sum is D * m_r and the mean m_r; every centred value is +-0.5, the variance 0.25, and with
# eps = 0.75 rstd = 1 / sqrt(1) = 1.  So y = sigma * gamma / 2 + beta, exact for small dyadic gamma and beta.
LN_EPS = 0.75
# Goes into every seed.  The smallest cases hold a handful of hashed values (3 x 4: six free signs, 1 x 64: two scale bytes) and
# can come out degenerate by chance; tests/test_exact_data_host.py demands its fault fractions at every shape, and this is the
# first salt under which all of them hold.
LN_SALT = 6
LN_PEAK_GAMMA, LN_PEAK_BETA = 15, 8      # |y| of a peak column is 15.5 or 0.5 by the row's sign; elsewhere |y| <= (7 + 6) / 2 = 6.5


def _ln_params(D, sd):
    """gamma (odd integer with a sign, 1..7) and beta (integer, -3..3), both times 2^-3..2^3 per 32-column block.  One hashed
    column of every block is a peak, gamma = +-15 and beta = +-8: the block's largest |y| is 15.5 * 2^k in the rows where
    sigma * gamma and beta agree in sign and at most 6.5 * 2^k in the others, so the E8M0 byte of the block (the exponent of
    amax / 448, rounded up: 15.5 and 6.5 lie on two sides of 14 = 448 / 32) depends on the row as well as on the block."""
    nblk = (D + 31) // 32
    blk = torch.arange(D, dtype=torch.int64) // 32
    g = (2 * ints("exact.ln.gamma", (D,), 0, 3, sd) + 1) * (2 * ints("exact.ln.gsign", (D,), 0, 1, sd) - 1)
    b = ints("exact.ln.beta", (D,), -3, 3, sd)
    width = torch.clamp(D - 32 * torch.arange(nblk, dtype=torch.int64), max=32)
    peak = 32 * torch.arange(nblk, dtype=torch.int64) + ints("exact.ln.peak", (nblk,), 0, 31, sd).long() % width
    g[peak] = LN_PEAK_GAMMA * (2 * ints("exact.ln.pgsign", (nblk,), 0, 1, sd) - 1)
    b[peak] = LN_PEAK_BETA * (2 * ints("exact.ln.pbsign", (nblk,), 0, 1, sd) - 1)
    scale = torch.ldexp(torch.ones(nblk), ints("exact.ln.pow", (nblk,), -3, 3, sd).to(torch.int32))[blk]
    return g * scale, b * scale


def ln_emulate(x, gamma, beta, eps):
    """The kernels' arithmetic in torch fp32: two-pass mean and variance (fp32 sums), 1 / sqrt(var + eps), one multiply-add chain."""
    x = x.float()
    D = x.shape[1]
    mean = x.sum(1, keepdim=True) / D
    d = x - mean
    rstd = 1.0 / torch.sqrt((d * d).sum(1, keepdim=True) / D + eps)
    return d * rstd * gamma.float() + beta.float(), mean, rstd


def ln_reference(x, gamma, beta, eps):
    """Plain LayerNorm over the last dimension in fp64."""
    x = x.double()
    mean = x.mean(1, keepdim=True)
    d = x - mean
    return d / torch.sqrt((d * d).mean(1, keepdim=True) + eps) * gamma.double() + beta.double()


def ln_case(M, D):
    """x (M, D), gamma (D,), beta (D,) fp32 and y (M, D) fp64, the closed form sigma * gamma / 2 + beta of LayerNorm(x) at
    eps = LN_EPS.  Asserts what makes y the exact answer of an fp32 kernel: balanced rows, mean m_r and rstd 1 bit for bit
    under ln_emulate, the emulation and the fp64 LayerNorm equal to the closed form, y unchanged by bf16 and fp16."""
    assert D % 4 == 0 and D >= 4
    sd = _shape_seed(M, D, LN_SALT)
    m = ints("exact.ln.mean", (M, 1), -6, 6, sd)
    h = 2 * ints("exact.ln.sigma", (M, D // 2), 0, 1, sd) - 1
    sigma = torch.cat([h, -h], 1)
    x = m + 0.5 * sigma
    gamma, beta = _ln_params(D, sd)
    y = sigma.double() * (gamma.double() / 2) + beta.double()
    assert torch.equal(x.sum(1, keepdim=True), D * m) and torch.equal(x.double().sum(1, keepdim=True), D * m.double())
    emu, mean, rstd = ln_emulate(x, gamma, beta, LN_EPS)
    assert torch.equal(mean, m) and torch.equal(rstd, torch.ones(M, 1)), (M, D)
    assert torch.equal(emu.double(), y) and torch.equal(ln_reference(x, gamma, beta, LN_EPS), y), (M, D)
    yf = y.float()
    assert torch.equal(yf.to(torch.bfloat16).double(), y) and torch.equal(yf.to(torch.float16).double(), y), (M, D)
    return x, gamma, beta, y


def ln_accum_case(M, D, S, bias=True):
    """Operands of hm_layernorm_accum whose sum is ln_case(M, D)'s x: x0 (M, D), parts (S, M, D) and bias (D,) or None, all
    hashed multiples of 0.5 (so every partial sum is exact in fp32), the last slab carrying the remainder.
    Returns x0, parts, bias, x, gamma, beta, y."""
    x, gamma, beta, y = ln_case(M, D)
    sd = _shape_seed(M, D, S)
    x0 = ints("exact.lnacc.x0", (M, D), -8, 8, sd) / 2
    b = ints("exact.lnacc.bias", (D,), -6, 6, sd) / 2 if bias else None
    parts = ints("exact.lnacc.part", (S, M, D), -8, 8, sd) / 2
    parts[S - 1] = x - x0 - parts[:S - 1].sum(0) - (b if bias else 0.0)
    total = x0.double() + parts.double().sum(0) + (b.double() if bias else 0.0)
    assert torch.equal(total, x.double()) and torch.equal(parts * 2, (parts * 2).round())
    assert (float(x0.abs().max()) + float(parts.abs().sum(0).max()) + _amax(b)) * 2 < EXACT_LIMIT
    return x0, parts, b, x, gamma, beta, y


# Rows for the accuracy test of the LayerNorm kernels against fp64: ordinary ones and the ones a careless kernel gets wrong.
LN_HOSTILE_KINDS = ("uniform", "mean_1000", "mean_-3000", "var_eps", "var_1e-3_eps", "outlier", "zero")
LN_ROWS_PER_KIND = 6
# Largest error of ln_emulate against fp64 per kind of row, in units of ln_error_unit, over D in LN_HOSTILE_D and both eps
# (measured by tests/test_exact_data_host.py::test_ln_error_multiples_are_the_measured_ones, which fails if one is exceeded or
# is more than twice what is measured); a kernel gets LN_KERNEL_MARGIN times that, because its reduction order differs.
LN_HOSTILE_D = [96, 320, 1280, 2048]
LN_HOSTILE_EPS = [1e-6, 1e-5]
LN_MULTIPLES = {"uniform": 1.6, "mean_1000": 1.0, "mean_-3000": 0.9, "var_eps": 1.7, "var_1e-3_eps": 2.3, "outlier": 1.9, "zero": 0.0}
LN_KERNEL_MARGIN = 4.0


def ln_hostile_rows(D, eps):
    """x (7 * LN_ROWS_PER_KIND, D), gamma, beta, kind index per row.  |x| <= 1e4: overflow of the squares is out of scope."""
    R = LN_ROWS_PER_KIND
    u = lambda tag, hw, center=0.0: synth.uniform("ln.hostile." + tag, (R, D), hw, center, seed=D)      # noqa: E731
    outlier = u("outlier", 3.0 ** 0.5)
    outlier[torch.arange(R), ints("ln.hostile.at", (R,), 0, D - 1, D).long()] = 1e4
    rows = [u("uniform", 3.0, 0.5), u("mean1000", 3.0 ** 0.5, 1000.0), u("mean-3000", 0.1 * 3.0 ** 0.5, -3000.0),
            u("vareps", (3.0 * eps) ** 0.5), u("var1e-3eps", (3.0e-3 * eps) ** 0.5), outlier, torch.zeros(R, D)]
    kind = torch.arange(len(rows)).repeat_interleave(R)
    gamma = synth.uniform("ln.hostile.gamma", (D,), 0.1, 1.0, seed=1)
    beta = synth.uniform("ln.hostile.beta", (D,), 0.1, 0.0, seed=2)
    return torch.cat(rows, 0), gamma, beta, kind


def ln_error_unit(x, gamma, eps):
    """(rows, 1) fp64: 2^-23 * (max|x - mean| / sqrt(var + eps) * max|gamma| + |mean| / sqrt(var + eps)), the size of one fp32
    rounding of the largest normalised value plus the share of one rounding of the mean."""
    x = x.double()
    mean = x.mean(1, keepdim=True)
    d = x - mean
    sd = torch.sqrt((d * d).mean(1, keepdim=True) + eps)
    return 2.0 ** -23 * (d.abs().amax(1, keepdim=True) / sd * float(gamma.abs().max()) + mean.abs() / sd)


def ln_error_bound(x, gamma, eps, kind, margin=LN_KERNEL_MARGIN):
    """(rows, 1) fp64 bound on |kernel - fp64| for fp32 output: margin * LN_MULTIPLES[kind of the row] * ln_error_unit."""
    mult = torch.tensor([LN_MULTIPLES[k] for k in LN_HOSTILE_KINDS], dtype=torch.float64)[kind][:, None]
    return margin * mult * ln_error_unit(x, gamma, eps)


def ulp16(ref, dtype):
    """One step of the 16-bit format at |ref|, from above: 2^-8 |ref| for bf16 (8 significant bits), 2^-11 |ref| for fp16 and
    never less than 2^-24, the spacing of fp16's subnormals."""
    return ref.abs() * 2.0 ** -8 if dtype == torch.bfloat16 else torch.clamp(ref.abs() * 2.0 ** -11, min=2.0 ** -24)


# ------------------------------------------------------------------------------------------------ the shapes of the GPU tests
# hm_layernorm: every D selects one width class of the row kernel on its unpaired or its paired ("full", D = MAXJ * 256) store
# path; the small M run one row per wave, the large ones 2, 3 and 3 (ln_large_m: 16 CUs + 1, 32 CUs + 5 ragged, 48 CUs whole)
LN_D = [4, 96, 252, 256, 260, 320, 512, 516, 768, 1024, 1028, 1276, 1280, 1284, 1536, 2044, 2048]
LN_M = [1, 3, 5, 197]
LN_LARGE_M_D = [96, 256, 512, 1280, 2048]
LN_HOST_CUS = 256                        # the CU count the host catalogue builds the large M with
LN_ACCUM_D = [4, 320, 512, 1280, 1284, 2048]
LN_ACCUM_M = [1, 5, 197]
LN_ACCUM_S = [1, 4, 5, 10]
LN_MX8_D = [32, 64, 256, 288, 512, 544, 1280, 1312, 1536, 2048]
LN_MX8_M = [1, 5, 197, 520]


def ln_large_m(cus):
    return [16 * cus + 1, 32 * cus + 5, 48 * cus]


def ln_shapes(cus=LN_HOST_CUS):
    return [(M, D) for D in LN_D for M in LN_M] + [(M, D) for D in LN_LARGE_M_D for M in ln_large_m(cus)]


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


# ------------------------------------------------------------------------------------------------ hm_linear_f32
# (M, N, K) of the decoder's small fp32 linear (csrc/decoder.hip: one 16 x 16 tile per workgroup, four waves splitting K in
# 16-wide blocks, a 4-deep prefetch loop entered while kb + 192 < K).  PROD: what forward.hip launches for synth.HamerConfig().
def linear_f32_prod():
    cfg = synth.HamerConfig()
    d, v = cfg.dec, cfg.vit
    nk = sorted({(d.dim, d.dim), (d.inner, d.dim), (d.dim, d.inner), (d.mlp_dim, d.dim), (d.dim, d.mlp_dim)})
    shapes = [(M, N, K) for (N, K) in nk for M in (1, 7, 64)]
    shapes += [(M, 112, d.dim) for M in (1, 7, 64)]                                  # the 112-wide head, ldo = 112
    shapes.append((2 * v.tokens, v.head_dim, v.embed_dim))                          # the token-merging metric, ldo = 80
    return shapes


LINEAR_F32_PROD = linear_f32_prod()
# EDGE: every M in {1, 15, 16, 17, 33} (row clamp, second blockIdx.y), N in {4, 12, 20, 80, 112} (the n >= N guard inside a
# tile; one lane group at 4) and K in {16, 48, 64, 208, 240, 256, 272, 464} at least twice.  K = 16: waves 1-3 add zeros; 48:
# wave 3 adds nothing; 208: only wave 0 enters the prefetch loop; 240, 256: the waves enter it one by one, 256 is one round
# and no tail; 272: a tail step for wave 0 after the round; 464: two rounds for waves 0 and 1.
LINEAR_F32_M = [1, 15, 16, 17, 33]
LINEAR_F32_N = [4, 12, 20, 80, 112]
LINEAR_F32_K = [16, 48, 64, 208, 240, 256, 272, 464]
LINEAR_F32_EDGE = [(1, 4, 16), (15, 12, 48), (16, 20, 64), (17, 80, 208), (33, 112, 240), (1, 12, 256), (15, 20, 272), (16, 80, 464),
                   (17, 112, 16), (33, 4, 48), (1, 20, 64), (15, 80, 208), (16, 112, 240), (17, 4, 256), (33, 12, 272), (1, 80, 464),
                   (15, 112, 16), (16, 4, 48), (17, 12, 64), (33, 20, 272), (33, 80, 256), (17, 20, 464)]
# leading dimensions wider than the row: one shape of whole tiles, one ragged in M, N and K (both are in the lists above)
LINEAR_F32_STRIDED = [(64, 512, 1024), (33, 20, 272)]


# ------------------------------------------------------------------------------------------------ token merging
# Metric rows whose bipartite matching is exact in fp32 whatever the summation order.  A token is +-m on c of the 80 channels,
# m in {1, 2, 3, 5} and c in {4, 16, 64}: the squared norm m^2 c is an integer, the norm m sqrt(c) an integer, every normalised
# value +-1 / sqrt(c) a power of two and every cosine a multiple of 1/64 of magnitude <= 1.  A token takes one of TOME_POOL
# (sign pattern, channel order) pairs, its support being the first c channels of that order, with up to three hashed sign
# flips inside the support: duplicates (cosine 1 whatever the magnitudes), near-duplicates and ties are plentiful.
TOME_HD = 80
TOME_POOL = 6
TOME_MAGNITUDES = [1, 2, 3, 5]
TOME_SUPPORTS = [4, 16, 64]
TOME_B = 3
TOME_D = [8, 320]
TOME_EXACT = [(192, 16), (192, 96), (191, 95), (161, 14), (129, 1), (17, 4), (3, 1), (2, 1)]      # (T, r)
# Goes into the seed of the case.  tests/test_exact_data_host.py states what the matching data must contain at every T >= 17
# (distinct scores, tied maxima, a crowded and an empty B token, a tie across the merge boundary, norms that matter); these
# are the first salts under which all of it holds.
TOME_SALT = {17: 2}
TOME_FILL = 3.0                           # what the columns around the metric hold in the wide layouts
TOME_LAYOUTS = ("ld80", "ld96", "hi_lo")


def tome_sizes_given(T):
    return T != 192


def tome_match_case(B, T, seed=0):
    """(B, T, 80) fp32 metric of small integers as described above; element (b, t) is a hash of b * T + t, so no crop repeats
    another."""
    sd = _shape_seed(B, T, seed)
    sign = 2 * ints("exact.tome.sign", (TOME_POOL, TOME_HD), 0, 1, sd) - 1
    order = torch.argsort(ints("exact.tome.order", (TOME_POOL, TOME_HD), 0, 1 << 20, sd), dim=1, stable=True)
    place = torch.argsort(order, dim=1)                                              # place[p, channel] = its position in order[p]
    p = ints("exact.tome.pool", (B, T), 0, TOME_POOL - 1, sd).long()
    c = torch.tensor(TOME_SUPPORTS)[ints("exact.tome.support", (B, T), 0, len(TOME_SUPPORTS) - 1, sd).long()]
    m = torch.tensor(TOME_MAGNITUDES, dtype=torch.float32)[ints("exact.tome.magnitude", (B, T), 0, len(TOME_MAGNITUDES) - 1, sd).long()]
    nflip = ints("exact.tome.nflip", (B, T), 0, 3, sd).long()
    at = ints("exact.tome.flip", (B, T, 3), 0, 63, sd).long() % c[..., None]          # positions inside the support
    s = sign[p].clone()                                                               # (B, T, 80)
    for k in range(3):
        ch = order[p].gather(2, at[..., k:k + 1])                                     # (B, T, 1) channel of flip k
        flip = torch.where(nflip[..., None] > k, -1.0, 1.0)
        s.scatter_(2, ch, s.gather(2, ch) * flip)
    metric = m[..., None] * s * (place[p] < c[..., None])
    assert metric.dtype == torch.float32 and metric.shape == (B, T, TOME_HD) and torch.equal(metric, metric.round())
    return metric


def tome_merge_case(B, T, D, with_size):
    """x (B, T, D) of integers in -50..50 and sizes (B, T) of integers in 1..4 (or None): every size-weighted sum of a merged
    group (at most 97 tokens) is an integer below 2^24."""
    sd = _shape_seed(B, T, D)
    x = ints("exact.tome.x", (B, T, D), -50, 50, sd)
    size = ints("exact.tome.size", (B, T), 1, 4, sd) if with_size else None
    assert 50 * 4 * (T // 2 + 2) < EXACT_LIMIT
    return x, size


def tome_metric_layout(metric, kind):
    """The metric as hm_tome_merge_metric is handed it: (buf (B * T, ld), first column, columns, lo_off).  The kernel gets the
    column slice buf[:, first:first + columns], row stride ld.  'ld80': the rows as they are.  'ld96': 80 columns from column 8
    of 96, TOME_FILL around them.  'hi_lo': ld = 176, the slice starts at column 4, hi = v + c in its columns 0..79 and
    lo = -c in its columns 88..167 for hashed integers c in -7..7 (hi + lo = v exactly), TOME_FILL everywhere else."""
    B, T, hd = metric.shape
    rows = metric.reshape(B * T, hd)
    if kind == "ld80":
        return rows.clone(), 0, hd, 0
    if kind == "ld96":
        buf = torch.full((B * T, 96), TOME_FILL)
        buf[:, 8:8 + hd] = rows
        return buf, 8, hd, 0
    assert kind == "hi_lo"
    c = ints("exact.tome.lo", (B * T, hd), -7, 7, _shape_seed(B, T))
    buf = torch.full((B * T, 176), TOME_FILL)
    buf[:, 4:4 + hd] = rows + c
    buf[:, 4 + 88:4 + 88 + hd] = -c
    assert torch.equal(buf[:, 4:4 + hd] + buf[:, 92:92 + hd], rows)
    return buf, 4, 88 + hd, 88


def tome_head_keys(metric, heads, dtype):
    """(B * T, 3 * heads * 80) qkv rows of `dtype` whose keys are metric + delta_h for hashed integers delta_h (-8..8, the
    last head's the negated sum of the others): their mean over the heads is the metric bit for bit.  q and v hold 1."""
    B, T, hd = metric.shape
    d = ints("exact.tome.delta", (B * T, heads - 1, hd), -8, 8, _shape_seed(B, T, heads))
    d = torch.cat([d, -d.sum(1, keepdim=True)], 1)
    k = metric.reshape(B * T, 1, hd) + d
    assert torch.equal(k.sum(1) / heads, metric.reshape(B * T, hd)) and torch.equal(k.to(dtype).float(), k)
    qkv = torch.ones(B * T, 3, heads, hd)
    qkv[:, 1] = k
    return qkv.reshape(B * T, 3 * heads * hd).to(dtype)


# ------------------------------------------------------------------------------------------------ SAR hand-mesh head
# csrc/sar.hip (f16 operands, fp32 accumulation, f16 or fp32 out) and csrc/sar_f32.hip: 128 x 128 tiles, a K loop of 32.
# SAIGB: (B, K): M = 6224 channels, N = 64 B positions (B = 1 is half an N tile, B = 3 a tile and a half); K = 512 runs through
# hm_sar_saigb, hm_sar_saigb_ch and hm_sar_saigb_f32, K = 1024 through hm_sar_saigb_ch alone.
SAR_NV, SAR_NJ, SAR_NT, SAR_CELLS, SAR_KG = 778, 21, 799, 1024, 544
SAR_SAIGB = [(1, 512), (3, 512), (1, 1024), (3, 1024)]
# L . X, M = K = 778: N = 8 (every column group of the f16 kernel clamps to column 0), one tile + 8, the two production
# widths at B = 1, B = 5 ragged; N = 4 and 132 are the fp32 kernel's N % 4 granularity.  ldl: production and one that adds a
# whole K step of zero Laplacian columns.
SAR_MIX_N = [8, 136, 544, 1024, 2720]
SAR_MIX_N_F32_ONLY = [4, 132]
SAR_MIX_LDL = [800, 832]
SAR_MIX_XROWS = 800                       # rows of the x buffer; rows 778 .. 799 hold NaN in the GPU test
# fc (M, N, K): one row, one column, one K step; one row and two columns into the second tile; an odd number of K steps; the two
# production layers; B = 3 rows with a ragged N
SAR_FC = [(1, 1, 32), (129, 130, 64), (257, 136, 96), (778, 1024, 544), (778, 1024, 1024), (2334, 200, 544)]
SAR_LEAKY = 0.1
F16_EXACT_INT = 2048.0                    # every integer of magnitude <= 2048 is an fp16 value


def sar_leaky(v):
    """LeakyReLU(0.1) as one fp32 multiply of the exact fp32 v (nothing here can contract into an FMA)."""
    assert v.dtype == torch.float32
    return torch.where(v > 0, v, v * torch.tensor(SAR_LEAKY, dtype=torch.float32))


def _f16_once(v):
    """v rounded once to fp16; asserts that the integers it holds (the positive half, and v before the LeakyReLU) are fp16 values."""
    h = v.half()
    pos = v > 0
    assert torch.equal(h.float()[pos], v[pos]) and float(v.abs().max()) <= F16_EXACT_INT
    return h


def sar_fc_case(M, N, K):
    """gemm_case(M, N, K) and the four expected outputs of the fc kernels: x (M, K), w (N, K), bias (N,), then
    {"f16_leaky": fp16, "f32": fp32 (hm_sar_linear out_f32 = 0 / 1), "f32_leaky", "f32_logits": fp32 (hm_sar_linear_f32 logits = 0 / 1)}."""
    x, w, b, _ = gemm_case(M, N, K)
    assert torch.equal(x.half().float(), x) and torch.equal(w.half().float(), w)
    v = x @ w.t() + b
    assert torch.equal(v.double(), x.double() @ w.double().t() + b.double())
    assert float(v.abs().max()) <= F16_EXACT_INT and torch.equal(v.half().float(), v), (M, N, K)
    lk = sar_leaky(v)
    return x, w, b, {"f16_leaky": _f16_once(lk), "f32": v, "f32_leaky": lk, "f32_logits": v}


def sar_graph(v, tmpl, B):
    """The SAIGB epilogue's scatter: v (64 B, 6224) [position b * 64 + p][channel m] -> the node-major graph (778, B, 544):
    channel m of position p of hand b at node m // 8, column (m % 8) * 64 + p; then the 3 template columns and 29 zeros."""
    g = torch.zeros(SAR_NV, B, SAR_KG, dtype=v.dtype)
    g[:, :, :512] = v.reshape(B, 64, SAR_NV, 8).permute(2, 0, 3, 1).reshape(SAR_NV, B, 512)
    g[:, :, 512:515] = tmpl.to(v.dtype)[:, None, :]
    return g


def sar_saigb_case(B, K):
    """feat (64 B, K) in -3..3 (NHWC rows), w (6224, K) in -2..2, bias (6224,) in -4..4 (gemm_case's x, w, bias), the template
    (778, 3) in -4..4, v = feat w^T + bias (64 B, 6224) exact, and the expected graphs {"f16", "f32"} (778, B, 544)."""
    M = 8 * SAR_NV
    feat, w, b, _ = gemm_case(64 * B, M, K)
    tmpl = ints("exact.sar.tmpl", (SAR_NV, 3), -4, 4, _shape_seed(B, K))
    v = feat @ w.t() + b
    assert float(v.abs().max()) <= F16_EXACT_INT and torch.equal(v.half().float(), v), (B, K)
    lk = sar_leaky(v)
    return feat, w, b, tmpl, v, {"f16": sar_graph(_f16_once(lk), tmpl, B), "f32": sar_graph(lk, tmpl, B)}


def sar_mix_case(N, ldl):
    """lap (778, ldl): a dense 778 x 778 of integers in -2..2 and zero columns 778 .. ldl - 1; x (778, N) in -3..3;
    y = lap[:, :778] x (778, N), exact in fp32 and unchanged by fp16."""
    assert ldl >= SAR_NV
    sd = _shape_seed(SAR_NV, N)
    lap = torch.zeros(SAR_NV, ldl)
    lap[:, :SAR_NV] = ints("exact.sar.lap", (SAR_NV, SAR_NV), -2, 2, sd)
    x = ints("exact.sar.x", (SAR_NV, N), -3, 3, sd)
    assert exact_bound(lap, x, SAR_NV) < EXACT_LIMIT
    y = lap[:, :SAR_NV] @ x
    assert torch.equal(y.double(), lap[:, :SAR_NV].double() @ x.double())
    assert float(y.abs().max()) <= F16_EXACT_INT and torch.equal(y.half().float(), y), (N, ldl)
    return lap, x, y


# ---- soft-argmax: "few-hot" logits.  Per (hand, vertex) row a hashed support of m in {1, 2, 4, .., 64} cells holds a hashed
# integer level l in -3..3 and every other cell l - 256; with beta >= 1 exp(beta (v - max)) is 1 on the support and 0 elsewhere
# (exp reaches fp32 zero at -104: 256 leaves a wide margin), p = 1 / m exactly and the three sums are short dyadic numbers in
# any order; with beta = 0 the row is uniform, p = 1 / 1024.  z logits are hashed integers in -8..8 at every cell.
SAR_SOFTARGMAX_B = [1, 3]
SAR_FEWHOT_GAP = 256
SAR_BETAS = [0.0, 1.0, 2.0, 4.0]
# Goes into the seed of the dense mesh2pose weights.  A dense joint row is sum_v W[j, v] (row v): its logits differ between cells
# by multiples of 256, so its softmax (beta >= 1) is uniform over the t cells that tie for the maximum.  With t = 3 or 5, 1 / t is
# not an fp32 value and the z sum, of magnitude up to 500 (half an ulp: 1.5e-5), cannot be held to the test's 1e-5 by any fp32
# kernel; the builder asserts that every such t is a power of two, and this is the first salt under which that holds at B = 1 and 3.
SAR_M2P_SALT = 32


def sar_fewhot_expect(lxy, lz, beta, wx, wy):
    """Closed form of SoftHeatmap + the coordinate sums on few-hot rows, float64: lxy, lz (..., 1024), beta (...,) -> (..., 3).
    The support of a row is where lxy is the row's maximum (every cell where beta = 0); asserts the gap to every other cell."""
    lxy, lz, beta = lxy.double(), lz.double(), beta.double()
    top = lxy.amax(-1, keepdim=True)
    supp = (lxy == top) | (beta[..., None] == 0)
    assert bool(((lxy <= top - SAR_FEWHOT_GAP) | supp).all()) and bool(((beta == 0) | (beta >= 1)).all())
    cnt = supp.sum(-1).double()
    mean = lambda t: (supp * t.double()).sum(-1) / cnt      # noqa: E731
    out = torch.stack([mean(wx) / 16 - 1, mean(wy) / 16 - 1, mean(lz)], -1)
    assert torch.equal(out.float().double(), out)
    return out


def sar_softmax_reference(lxy, lz, beta, wx, wy):
    """The same in plain float64 softmax, for rows that are not few-hot: (..., 1024) -> (..., 3)."""
    p = torch.softmax(lxy.double() * beta.double()[..., None], -1)
    return torch.stack([(p * wx.double()).sum(-1) / 16 - 1, (p * wy.double()).sum(-1) / 16 - 1, (p * lz.double()).sum(-1)], -1)


def sar_softargmax_case(B, m2p):
    """Operands and expectations of hm_sar_softargmax.  m2p = 'dense': mesh2pose weights (21, 778) of hashed integers in -2..2;
    'onehot': row j picks one hashed vertex v_j with weight 1; integer biases either way.  Returns a dict: lxy, lz (B, 778, 1024)
    fp32; w_xy, b_xy, w_z, b_z; beta (799,), wx, wy (1024,); jxy, jz (B, 21, 1024) the exact integer joint logits; coords
    (B, 799, 3) float64, fp32-representable in its exact part: all rows for 'onehot', rows 0..777 for 'dense', whose joint rows
    are the float64 softmax of the joint logits."""
    sd = _shape_seed(B, SAR_NT)
    NV, NJ, C = SAR_NV, SAR_NJ, SAR_CELLS
    m = torch.ldexp(torch.ones(B, NV), ints("exact.sar.m", (B, NV), 0, 6, sd).to(torch.int32)).long()
    rank = torch.argsort(torch.argsort(ints("exact.sar.cells", (B, NV, C), 0, 1 << 20, sd), dim=2, stable=True), dim=2)
    level = ints("exact.sar.level", (B, NV), -3, 3, sd)
    lxy = torch.where(rank < m[..., None], level[..., None], level[..., None] - SAR_FEWHOT_GAP)
    lz = ints("exact.sar.z", (B, NV, C), -8, 8, sd)
    beta = torch.tensor(SAR_BETAS)[ints("exact.sar.beta", (SAR_NT,), 0, len(SAR_BETAS) - 1, 0).long()]
    cell = torch.arange(C)
    wx, wy = (cell % 32).float(), (cell // 32).float()
    if m2p == "dense":
        w_xy, w_z = ints("exact.sar.m2p.xy", (NJ, NV), -2, 2, SAR_M2P_SALT), ints("exact.sar.m2p.z", (NJ, NV), -2, 2, SAR_M2P_SALT)
    else:
        assert m2p == "onehot"
        pick = ints("exact.sar.m2p.pick", (NJ,), 0, NV - 1, 0).long()
        w_xy = torch.zeros(NJ, NV)
        w_xy[torch.arange(NJ), pick] = 1.0
        w_z = w_xy.clone()
    b_xy, b_z = ints("exact.sar.m2p.bxy", (NJ,), -4, 4, 0), ints("exact.sar.m2p.bz", (NJ,), -4, 4, 0)
    assert NV * float(w_xy.abs().max()) * float(lxy.abs().max()) + 4 < EXACT_LIMIT
    jxy = torch.einsum("jv,bvc->bjc", w_xy, lxy) + b_xy[None, :, None]
    jz = torch.einsum("jv,bvc->bjc", w_z, lz) + b_z[None, :, None]
    assert torch.equal(jxy.double(), torch.einsum("jv,bvc->bjc", w_xy.double(), lxy.double()) + b_xy.double()[None, :, None])
    assert torch.equal(jz.double(), torch.einsum("jv,bvc->bjc", w_z.double(), lz.double()) + b_z.double()[None, :, None])
    vert = sar_fewhot_expect(lxy, lz, beta[:NV].expand(B, NV), wx, wy)
    if m2p == "onehot":
        joint = sar_fewhot_expect(jxy, jz, beta[NV:].expand(B, NJ), wx, wy)
    else:
        ties = (jxy == jxy.amax(-1, keepdim=True)).sum(-1)
        assert bool(((ties & (ties - 1)) == 0)[:, beta[NV:] > 0].all()), ("tied maxima of a dense joint row", ties.tolist())
        joint = sar_softmax_reference(jxy, jz, beta[NV:].expand(B, NJ), wx, wy)
    return {"lxy": lxy, "lz": lz, "w_xy": w_xy, "b_xy": b_xy, "w_z": w_z, "b_z": b_z, "beta": beta, "wx": wx, "wy": wy,
            "jxy": jxy, "jz": jz, "coords": torch.cat([vert, joint], 1)}


# ---- hm_sar_postprocess on dyadic data: every product and sum below is exact in fp32 (and in the double uvd -> xyz step), so
# neither FMA contraction nor operation order can change a bit.
SAR_POST_B, SAR_POST_P = 5, 256
SAR_POST_IMG = (1024, 512)                                         # width, height: the integer halves are powers of two
SAR_POST_K = (1024.0, 512.0, 512.0, 256.0)                         # fx, fy, fu, fv
SAR_POST_MAPS = [(7 + 16 * 8 + 5, 64, 32), (7, 16, 8)]            # (offset, width, height) of the two depth maps in one buffer
SAR_POST_DEPTH_LEN = 7 + 16 * 8 + 5 + 64 * 32 + 3
# per hand: bb2img (2 x 3), depth_box, flip, root, depth map (index into SAR_POST_MAPS or None), (u, v) of row 778 in patch
# pixels, and where the un-flipped row 778 must land in its map: "inside", "border" (x0 = -1 or x0 + 1 = W) or "outside"
SAR_POST_HANDS = [
    dict(t=[[0.5, 0.0, 100.0], [0.0, 0.5, 40.0]], box=0.25, flip=0, root=0.625, map=0, uv=(208, 120), lands="inside"),
    dict(t=[[1.0, 0.25, -30.0], [0.0, 1.0, 17.0]], box=0.5, flip=1, root=1.375, map=None, uv=(100, 60), lands=None),
    dict(t=[[2.0, 0.0, 500.0], [0.25, 1.0, -9.0]], box=0.25, flip=1, root=0.875, map=1, uv=(252, 104), lands="border"),
    dict(t=[[0.25, 0.5, 3.0], [0.5, 0.0, 64.0]], box=0.5, flip=0, root=2.5, map=0, uv=(-128, -128), lands="outside"),
    dict(t=[[1.0, 0.0, 256.0], [0.0, 2.0, -100.0]], box=0.25, flip=0, root=0.3125, map=None, uv=(40, 360), lands=None),
]


def sar_bilinear(depth, W, H, gx, gy):
    """grid_sample(bilinear, zeros, align_corners=False) of the (H, W) map at one normalised point, in float64; also returns
    (x0, y0), the top-left cell of the footprint."""
    import math
    ix, iy = ((gx + 1) * W - 1) / 2, ((gy + 1) * H - 1) / 2
    x0, y0 = math.floor(ix), math.floor(iy)
    tx, ty = ix - x0, iy - y0
    acc = 0.0
    for dy in (0, 1):
        for dx in (0, 1):
            x, y = x0 + dx, y0 + dy
            if 0 <= x < W and 0 <= y < H:
                acc += (tx if dx else 1 - tx) * (ty if dy else 1 - ty) * float(depth[y * W + x])
    return acc, (x0, y0)


def sar_post_inputs():
    """coords (5, 799, 3) fp32: xy hashed multiples of 1/64 in [-1, 1), z hashed multiples of 1/64 in [-8, 8], row 778's xy set so
    that it lands where SAR_POST_HANDS says; depth: one buffer of hashed integers 0..15 holding both maps."""
    B = SAR_POST_B
    coords = torch.cat([ints("exact.sar.post.xy", (B, SAR_NT, 2), -64, 63, 0) / 64, ints("exact.sar.post.z", (B, SAR_NT, 1), -512, 512, 0) / 64], 2)
    for b, h in enumerate(SAR_POST_HANDS):
        coords[b, SAR_NV, 0], coords[b, SAR_NV, 1] = h["uv"][0] / SAR_POST_P - 0.5, h["uv"][1] / SAR_POST_P - 0.5
    depth = ints("exact.sar.post.depth", (SAR_POST_DEPTH_LEN,), 0, 15, 0)
    return coords, depth


def sar_post_expect(coords, depth, hands=None, with_root=True, with_depth=True, fault=None):
    """float64 statement of post_processing plus run's depth-image root for the hands of SAR_POST_HANDS (or `hands`):
    -> uvd, xyz (B, 799, 3) float64 and the per-hand root.  `fault` (tests/test_exact_data_host.py) names one deliberate mistake."""
    hands = SAR_POST_HANDS if hands is None else hands
    Wi, Hi = SAR_POST_IMG
    fx, fy, cu, cv = SAR_POST_K
    P = SAR_POST_P
    c = coords.double()
    uvd, xyz, roots = torch.empty_like(c), torch.empty_like(c), []
    for b, h in enumerate(hands):
        t = torch.tensor(h["t"], dtype=torch.float64)
        u, v = (c[b, :, 0] + 0.5) * P, (c[b, :, 1] + 0.5) * P
        fu, fv = t[0, 0] * u + t[0, 1] * v + t[0, 2], t[1, 0] * u + t[1, 1] * v + t[1, 2]
        r = h["root"] if with_root else 0.0
        if h["map"] is not None and with_depth:
            off, W, H = SAR_POST_MAPS[h["map"]]
            off = h.get("off", off)
            su, sv = float(fu[SAR_NV]), float(fv[SAR_NV])                 # row 778, NOT un-flipped
            if fault == "row 778 un-flipped before sampling" and h["flip"]:
                su = Wi - su - 1
            gx, gy = su / (Wi // 2) - 1, sv / (Hi // 2) - 1
            if fault == "x and y of the sample swapped":
                gx, gy = gy, gx
            if fault == "depth_w and depth_h swapped":
                W, H = H, W
            r, _ = sar_bilinear(depth[off:], W, H, gx, gy)
        if h["flip"] and fault != "flip ignored":
            fu = Wi - fu - 1
        z = c[b, :, 2] * h["box"] + r
        uvd[b] = torch.stack([fu, fv, z], 1)
        xyz[b] = torch.stack([(fu - cu) * z / fx, (fv - cv) * z / fy, z], 1)
        roots.append(r)
    return uvd, xyz, roots


def sar_post_case(with_root=True, with_depth=True):
    """coords, depth, the hand table and the expected uvd, xyz (fp32).  Asserts that row 778 of each depth hand lands where
    its entry says and that every expected value is an fp32 value."""
    coords, depth = sar_post_inputs()
    uvd, xyz, _ = sar_post_expect(coords, depth, with_root=with_root, with_depth=with_depth)
    Wi, Hi = SAR_POST_IMG
    seen = set()
    for b, h in enumerate(SAR_POST_HANDS):
        if h["map"] is None:
            continue
        off, W, H = SAR_POST_MAPS[h["map"]]
        t = torch.tensor(h["t"], dtype=torch.float64)
        su, sv = (t @ torch.tensor([h["uv"][0], h["uv"][1], 1.0], dtype=torch.float64)).tolist()
        _, (x0, y0) = sar_bilinear(depth[off:], W, H, su / (Wi // 2) - 1, sv / (Hi // 2) - 1)
        inx, iny = [0 <= x < W for x in (x0, x0 + 1)], [0 <= y < H for y in (y0, y0 + 1)]
        lands = "inside" if all(inx) and all(iny) else "outside" if not (any(inx) and any(iny)) else "border"
        assert lands == h["lands"], (b, lands, x0, y0)
        assert lands != "border" or (x0 == -1 or x0 + 1 == W), (b, x0)
        assert off + W * H <= SAR_POST_DEPTH_LEN
        seen.add(lands)
    assert seen == {"inside", "border", "outside"} and sum(h["flip"] for h in SAR_POST_HANDS) == 2
    assert torch.equal(uvd.float().double(), uvd) and torch.equal(xyz.float().double(), xyz)
    return coords, depth, SAR_POST_HANDS, uvd.float(), xyz.float()


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
