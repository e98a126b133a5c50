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
