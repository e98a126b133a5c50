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

The kernels behind the networks (sections "MANO tail", "Detect decode", "RootNet layout kernels") have data and rules of their
own: a dyadic MANO model with signed-permutation rotations, for which mano_rule asserts stage by stage that every sum is exact
in any order; three-valued logits whose fp32 sigmoid is exactly 1/2, 1 or 0 for the decode; integer features over a
power-of-two HW for the pooled linear layer; values every output type holds for the two layout kernels.

The fp8 GEMMs run all three epilogues on the exact integers (fp8_epilogue_case): hashed integer bias and residual for the fp32 and
bf16 outputs, and for GELU -> MXFP8 a bias that keeps every |v| >= 16, where the GELU is exactly max(v, 0), with block maxima on
both sides of 448 2^k.  The attention kernels (section "attention") get code-book data whose softmax is exactly few-hot: P is 1
on the m in {1, 2, 4} keys of a hashed group and 0 elsewhere, so the output is one rounding of sum / m.

Plain helper module (imported like sar_rule.py); torch and numpy on the CPU only, nothing here touches the compiled library.
"""
import numpy as np
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


def fp8_case(M, N, K, ws_range=1):
    """MXFP8 operands whose every product and sum is exact: xi (M,K) in -4..4 and wi (N,K) in -3..3 (integers that e4m3
    holds exactly), E8M0 block scales xs (K/32, M) of 2^-1..2^2 and per-row weight scales ws (N,) of 2^-1..2^1 (ws_range = 2:
    2^-2..2^2).  Returns x8, xs, w8, ws (the bytes and scales the kernel takes) and xi, wi (the same values as fp32)."""
    sd = _shape_seed(M, N, K)
    xi = ints("exact.fp8.x", (M, K), -4, 4, sd)
    wi = ints("exact.fp8.w", (N, K), -3, 3, sd)
    xs = (127 + ints("exact.fp8.xs", (K // 32, M), -1, 2, sd)).to(torch.uint8)
    ws = torch.ldexp(torch.ones(N), ints("exact.fp8.ws", (N,), -ws_range, ws_range, sd).to(torch.int32))
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


FP8_BIAS_RANGE, FP8_RESID_RANGE = 32, 510
FP8_GELU_EXACT = 16.0                     # |v| >= 16: exp2(-0.5 log2e v^2) <= 2^-184 is zero, both GELUs give max(v, 0) exactly
FP8_ZERO_BLOCKS = 5                       # about one 32-column block in five has a negative bias throughout and comes out all zero
# In the seeds of bias, resid and the GELU bias, as LN_SALT; and the exponent range of ws in these cases.  With ws in 2^-1..2^1
# the fault "row scales rotated" stays under 40 % of the GELU -> MXFP8 bytes at most shapes whatever the salt; with 2^-2..2^2 this
# is the first salt under which every listed shape meets every fault fraction of tests/test_exact_data_host.py.
FP8_SALT = 17
FP8_EPILOGUE_WS_RANGE = 2


def fp8_epilogue_case(M, N, K):
    """fp8_case plus what the three epilogues of hm_gemm_fp8 need to be exact, as a dict:
    x8, xs, w8, ws, xi, wi   the operands of fp8_case(M, N, K, FP8_EPILOGUE_WS_RANGE);
    acc (M, N) fp64           the scaled product, ws applied;
    bias (N,), resid (M, N)   hashed integers in +-FP8_BIAS_RANGE and +-FP8_RESID_RANGE: STORE expects acc + bias rounded once
                              to bf16, RESID_F32 expects acc + bias + resid, every sum exact in fp32 (asserted);
    gelu_bias (N,)            sign_n (448 2^kb - off): kb hashed per 32-column block in k0 .. k0 + 2 with
                              k0 = ceil(log2((A + 16 + 2 sigma) / 448)), off = round(1.6 sigma), A and sigma the maximum and
                              the standard deviation of |acc|; sign_n hashed per column and negative over whole blocks for
                              about a fifth of them.  v = acc + gelu_bias has |v| >= 16 everywhere (asserted), where the GELU is
                              exactly max(v, 0), and the block maxima straddle 448 2^kb, so the scale bytes depend on the row
                              and on the block; an all-negative block is all zero with the scale byte 0;
    positive (N,) bool        the columns whose bias is positive."""
    x8, xs, w8, ws, xi, wi = fp8_case(M, N, K, FP8_EPILOGUE_WS_RANGE)
    sd = _shape_seed(M, N, K, FP8_SALT)
    acc = fp8_reference(xi, xs, wi, ws)
    bias = ints("exact.fp8.bias", (N,), -FP8_BIAS_RANGE, FP8_BIAS_RANGE, sd)
    resid = ints("exact.fp8.resid", (M, N), -FP8_RESID_RANGE, FP8_RESID_RANGE, sd)
    sx = torch.ldexp(torch.ones(()), xs.to(torch.int32) - 127)
    unit = float(sx.min()) * float(ws.min())
    bound = exact_bound(xi, wi, K, bias, resid, scale=float(sx.max()) * float(ws.max()), unit=unit)
    assert bound < EXACT_LIMIT, (M, N, K, bound)
    for t in (acc + bias.double(), acc + bias.double() + resid.double()):
        assert torch.equal(t.float().double(), t)
    a = acc.abs()
    A, sigma = float(a.max()), float(a.std())
    k0 = int(np.ceil(np.log2((A + FP8_GELU_EXACT + 2 * sigma) / 448.0)))
    off = float(round(1.6 * sigma))
    nblk = N // 32
    kb = (k0 + ints("exact.fp8.gelu.kb", (nblk,), 0, 2, sd)).to(torch.int32).repeat_interleave(32)
    sign = 2 * ints("exact.fp8.gelu.sign", (N,), 0, 1, sd) - 1
    dead = (ints("exact.fp8.gelu.dead", (nblk,), 0, FP8_ZERO_BLOCKS - 1, sd) == 0).repeat_interleave(32)
    sign = torch.where(dead, -torch.ones(N), sign)
    gb = sign * (torch.ldexp(torch.full((N,), 448.0), kb) - off)
    v = acc + gb.double()
    assert float(v.abs().min()) >= FP8_GELU_EXACT, (M, N, K, float(v.abs().min()))
    assert torch.equal(v.float().double(), v) and float(v.abs().max()) / unit < EXACT_LIMIT
    return {"x8": x8, "xs": xs, "w8": w8, "ws": ws, "xi": xi, "wi": wi, "acc": acc, "bias": bias, "resid": resid,
            "gelu_bias": gb, "positive": sign > 0}


def fp8_gelu_expect(v):
    """(bytes (M, N), scales (N/32, M)) of GELU -> MXFP8 on v with |v| >= FP8_GELU_EXACT: the oracle quantiser on max(v, 0)."""
    from oracle import fp8_ref as Q
    v = v.float()
    return Q.mx8_quantize(torch.where(v > 0, v, torch.zeros_like(v)))


def fp8_unsigned_zero(b):
    """e4m3 bytes with -0 (0x80) written as +0: the kernels' GELU gives +0 where torch's gives -0."""
    return torch.where(b == 0x80, torch.zeros_like(b), b)


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
# hm_gemm_fp8 with its three epilogues: the one-tile kernel (HM_OPT_FP8_ONE_TILE where a shape would go persistent) ...
GEMM_FP8_ONE_TILE = [(16, 64, 128), (240, 192, 256), (272, 320, 384), (528, 576, 128), (256, 256, 5120), (768, 768, 1280)]
# ... and the persistent one: (M, N, K, HM_OPT_FP8P_GRID settings).  (768, 768, 384) on 8 workgroups: 9 tiles of three K-steps,
# one workgroup takes two with the ring parity flipped between them; (1024, 1280, 384): 20 tiles, XCD runs of 3 and 2
GEMM_FP8_PERSISTENT = [(512, 1024, 256, (0,)), (768, 768, 384, (8,)), (1024, 1280, 384, (8,)), (1280, 1024, 1280, (8, 16))]
GEMM_FP8_WIDE = [(272, 320, 384), (768, 768, 384)]                        # run with wide leading dimensions
GEMM_FP8_NO_BIAS = [(512, 1024, 256), (272, 320, 384)]
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


# ------------------------------------------------------------------------------------------------ MANO tail
# csrc/mano.hip on a dyadic model: every model parameter is a hashed integer over a power-of-two quantum, betas are small
# integers and every joint rotation is one of the 24 proper signed-permutation matrices, so every intermediate of the kernel
# is an fp32 value whatever the order of a sum and with or without FMA contraction.  mano_rule states the operation in
# float64 and asserts exactly that, stage by stage; the camera tail is the kernel's sequence of single fp32 operations.
MANO_B = [1, 5, 67]
MANO_V = [745, 778, 800]                  # the API's edges (744 < n_verts <= 800) and MANO's own count
MANO_NCHUNK = 4                           # workgroups (vertex ranges) per hand
MANO_TIP_OWNER = (3, 1, 2, 2, 3)          # the range that skins tip vertex (744, 320, 443, 554, 671), the same at all three V
MANO_FOCAL, MANO_IMAGE = 5000.0, 256.0
MANO_C0 = 625.0 / 16.0                    # image_size * c0 = 10000 / 2^m: the + 1e-9f is absorbed and tz = 2^m
MANO_DEGENERATE = (5, 778)                # (B, V) of the degenerate-pose case
MANO_DEGENERATE_JOINTS = {"a1 = 0": (0, 4), "a2 = t a1": (0, 8)}       # (hand, joint)
MANO_T = [0.5, -0.5, 1.0, -1.0, 1.5, -1.5, 3.0, -3.0]
MANO_LBS_PATTERNS = [[1.0, 0.0, 0.0, 0.0], [0.5, 0.5, 0.0, 0.0], [0.5, 0.25, 0.25, 0.0], [0.25, 0.25, 0.25, 0.25]]
F32_TINY = float(np.float32(1e-12))       # the kernel's norm floor, 1e-12f
MANO_FAULTS = ["wrong parent table", "joint map rotated", "tips off by one", "posedirs as [3V][135]", "shapedirs as [10][3V]",
               "rotation transposed", "pose feature from joint 0", "lbs_weights as [16][V]", "joints from v_posed", "A without G J",
               "one range unposed", "child before parent", "cam columns rotated"]
MANO_UNPOSED_RANGE = 1


def mano_ranges(V):
    """The four vertex ranges of the kernel: [k * ceil(V / 4), min(V, (k + 1) * ceil(V / 4)))."""
    vper = (V + MANO_NCHUNK - 1) // MANO_NCHUNK
    return [(k * vper, min(V, (k + 1) * vper)) for k in range(MANO_NCHUNK)]


def mano_rotation_table():
    """The 24 proper signed-permutation matrices as (i, s1, j, s2): columns b1 = s1 e_i, b2 = s2 e_j, b3 = b1 x b2; and which of
    them are symmetric (10 are: a transposed matrix passes on those)."""
    table = [(i, s1, (i + dj) % 3, s2) for i in range(3) for dj in (1, 2) for s1 in (1, -1) for s2 in (1, -1)]
    sym = []
    for i, s1, j, s2 in table:
        b1, b2 = torch.zeros(3), torch.zeros(3)
        b1[i], b2[j] = s1, s2
        m = torch.stack([b1, b2, torch.linalg.cross(b1, b2)], 1)
        assert abs(float(torch.linalg.det(m)) - 1) < 1e-6
        sym.append(bool(torch.equal(m, m.t())))
    return table, sym


def mano_exact_model(V, seed=0):
    """v_template k / 64 (|k| <= 8), shapedirs k / 64 (|k| <= 2), posedirs k / 64 (|k| <= 1); a J_regressor row is eight hashed
    vertices of weight 1 / 8; an lbs_weights row is one of MANO_LBS_PATTERNS on four hashed joints (weights add where they meet)."""
    sd = _shape_seed(V, seed)
    mp = {"v_template": ints("exact.mano.vt", (V, 3), -8, 8, sd) / 64, "shapedirs": ints("exact.mano.sd", (V, 3, 10), -2, 2, sd) / 64,
          "posedirs": ints("exact.mano.pd", (135, 3 * V), -1, 1, sd) / 64}
    pick = ints("exact.mano.jreg", (16, 8), 0, V - 1, sd).long()
    mp["J_regressor"] = torch.zeros(16, V).scatter_add_(1, pick, torch.full((16, 8), 0.125))
    pat = torch.tensor(MANO_LBS_PATTERNS)[ints("exact.mano.lbs.pattern", (V,), 0, 3, sd).long()]
    mp["lbs_weights"] = torch.zeros(V, 16).scatter_add_(1, ints("exact.mano.lbs.joint", (V, 4), 0, 15, sd).long(), pat)
    assert torch.equal(mp["J_regressor"].sum(1), torch.ones(16)) and torch.equal(mp["lbs_weights"].sum(1), torch.ones(V))
    owner = tuple(next(k for k, (lo, hi) in enumerate(mano_ranges(V)) if lo <= t < hi) for t in synth.MANO_TIP_VERTS)
    assert owner == MANO_TIP_OWNER and V > max(synth.MANO_TIP_VERTS), (V, owner)
    assert V != 745 or synth.MANO_TIP_VERTS[0] == mano_ranges(V)[3][1] - 1        # tip 744: the last vertex of the last workgroup
    return mp


def mano_exact_case(B, V, seed=0, degenerate=False):
    """(model, pose6d (B, 96), betas (B, 10), cam (B, 3), rot (B, 16) indices into mano_rotation_table).  Joint (b, j) takes a
    hashed rotation -- three in four from the 14 asymmetric ones -- that differs from every ancestor's in its finger and from
    hand b - 1's at the same joint, so hands 0 and 1 differ at every level of every finger and no parent / child mix-up is
    absorbed.  Its 6-D code is not normalised: a1 = s1 2^p e_i, a2 = s2 2^q e_j + t e_i with t != 0 on a hashed half.  cam:
    c0 = MANO_C0 / 2^m, c1 and c2 multiples of 1 / 64; the last row of a batch has c0 = 0 (a lone hand keeps an ordinary
    camera).  degenerate: MANO_DEGENERATE_JOINTS get a1 = 0 (and t = 0) and a2 = 1.5 a1."""
    sd = _shape_seed(B, V, seed)
    table, sym = mano_rotation_table()
    asym = [k for k in range(24) if not sym[k]]
    h = ints("exact.mano.rot", (B, 16), 0, (1 << 20) - 1, sd).long().tolist()
    rot = [[0] * 16 for _ in range(B)]
    for b in range(B):
        for j in range(16):
            cand = list(range(24)) if h[b][j] % 4 == 0 else asym
            banned, a = set(), synth.MANO_PARENTS[j]
            while a >= 0:
                banned.add(rot[b][a])
                a = synth.MANO_PARENTS[a]
            if b:
                banned.add(rot[b - 1][j])
            k = (h[b][j] // 4) % len(cand)
            while cand[k] in banned:
                k = (k + 1) % len(cand)
            rot[b][j] = cand[k]
    p = ints("exact.mano.p", (B, 16), -1, 2, sd)
    q = ints("exact.mano.q", (B, 16), -2, 1, sd)
    t = torch.tensor(MANO_T)[ints("exact.mano.t", (B, 16), 0, len(MANO_T) - 1, sd).long()] * ints("exact.mano.t.on", (B, 16), 0, 1, sd)
    pose = torch.zeros(B, 16, 6)
    for b in range(B):
        for j in range(16):
            i, s1, jj, s2 = table[rot[b][j]]
            pose[b, j, i] = s1 * 2.0 ** float(p[b, j])
            pose[b, j, 3 + jj] = s2 * 2.0 ** float(q[b, j])
            pose[b, j, 3 + i] = t[b, j]
    if degenerate:
        b, j = MANO_DEGENERATE_JOINTS["a1 = 0"]
        pose[b, j, :3] = 0.0
        pose[b, j, 3 + table[rot[b][j]][0]] = 0.0
        b, j = MANO_DEGENERATE_JOINTS["a2 = t a1"]
        pose[b, j, 3:] = 1.5 * pose[b, j, :3]
    else:
        assert float((t != 0).float().mean()) > 0.25 or B == 1
    betas = ints("exact.mano.betas", (B, 10), -2, 2, sd)
    cam = torch.cat([MANO_C0 / 2.0 ** ints("exact.mano.cam.m", (B, 1), 0, 3, sd), ints("exact.mano.cam.xy", (B, 2), -64, 64, sd) / 64], 1)
    if B > 1:
        cam[B - 1, 0] = 0.0
    return mano_exact_model(V, seed), pose.reshape(B, 96), betas, cam, torch.tensor(rot)


def _stage(exact, what, q, eq, *factors, add=()):
    """einsum(eq, factors) + the addends, in float64.  With `exact` it asserts what makes an fp32 kernel's result the same in any
    summation order and with or without FMA contraction: every factor is a multiple of its own quantum, the product of those
    quanta and every addend a multiple of q -- so every term of every sum is a multiple of q -- and sum |terms| / q < 2^24."""
    val = torch.einsum(eq, *[t for t, _ in factors])
    for a in add:
        val = val + a
    if exact:
        qq = 1.0
        for t, qt in factors:
            assert torch.equal(t / qt, (t / qt).round()), (what, "a factor off its quantum", qt)
            qq *= qt
        assert (qq / q) == round(qq / q) and qq >= q, (what, qq, q)
        mag = torch.einsum(eq, *[t.abs() for t, _ in factors])
        for a in add:
            assert torch.equal(a / q, (a / q).round()), (what, "an addend off the quantum", q)
            mag = mag + a.abs()
        assert float(mag.max()) / q < EXACT_LIMIT, (what, float(mag.max()) / q)
    return val


def mano_rot6d_rule(pose6d, exact=True):
    """The kernel's Gram-Schmidt step by step in float64 -> (N, 3, 3), columns (b1, b2, b1 x b2); norms floored at 1e-12f.
    `exact`: every squared norm is 0 or the square of an fp32 number, and every value on the way is an fp32 value."""
    x = pose6d.double().reshape(-1, 6)
    a1, a2 = x[:, :3], x[:, 3:]

    def unit(v, what):
        ss = (v * v).sum(1, keepdim=True)
        n = ss.sqrt()
        if exact:
            assert torch.equal(n * n, ss) and torch.equal(n.float().double(), n) and float(ss.max()) * 2.0 ** 16 < EXACT_LIMIT, what
            assert torch.equal(v * v * 2.0 ** 16, (v * v * 2.0 ** 16).round()), what
        out = v / n.clamp_min(F32_TINY)
        assert not exact or torch.equal(out.float().double(), out), what
        return out

    b1 = unit(a1, "a1")
    d = (b1 * a2).sum(1, keepdim=True)
    u = a2 - d * b1
    if exact:
        for t in (b1 * a2, d, d * b1, u):
            assert torch.equal(t * 256, (t * 256).round()) and float(t.abs().max()) * 256 < EXACT_LIMIT
    b2 = unit(u, "a2 - (b1 . a2) b1")
    return torch.stack([b1, b2, torch.linalg.cross(b1, b2, dim=1)], -1) + 0.0       # + 0.0: no negative zeros


def mano_rule(mp, pose6d, betas, cam, focal=MANO_FOCAL, image_size=MANO_IMAGE, fault=None, exact=True):
    """hm_mano_forward stated plainly -> fp32 rotmats (B, 16, 3, 3), verts (B, V, 3), joints (B, 21, 3), cam_t (B, 3),
    kp2d (B, 21, 2).  Everything up to the joints is float64 through _stage, which (exact=True) asserts the exactness of
    v_shaped, J, the pose feature, v_posed, the chain, A, the blended transform and the skinned vertex.  The camera tail is the
    kernel's own sequence of single, correctly rounded fp32 operations in numpy.float32: tz = 2 focal / (image_size c0 + 1e-9f)
    (the product is exact on this data, so a contracted FMA rounds the same), px = jx + c1, pz = jz + tz,
    (px / pz) * (focal / image_size).  `fault` names one deliberate mistake of MANO_FAULTS (tests/test_exact_data_host.py)."""
    assert fault is None or fault in MANO_FAULTS
    B, V = pose6d.shape[0], mp["v_template"].shape[0]
    vt, sd, pd, jr, w = (mp[k].double() for k in ("v_template", "shapedirs", "posedirs", "J_regressor", "lbs_weights"))
    if fault == "posedirs as [3V][135]":
        pd = pd.reshape(3 * V, 135).t()
    if fault == "shapedirs as [10][3V]":
        sd = sd.reshape(10, 3 * V).t().reshape(V, 3, 10)
    if fault == "lbs_weights as [16][V]":
        w = w.reshape(16, V).t()
    parents = list(range(-1, 15)) if fault == "wrong parent table" else synth.MANO_PARENTS
    R = mano_rot6d_rule(pose6d, exact).reshape(B, 16, 3, 3)
    if fault == "rotation transposed":
        R = R.transpose(-1, -2)
    eye = torch.eye(3, dtype=torch.float64)
    vs = _stage(exact, "v_shaped", 1 / 64, "vcl,bl->bvc", (sd, 1 / 64), (betas.double(), 1.0), add=(vt[None],))
    first = 0 if fault == "pose feature from joint 0" else 1
    pf = _stage(exact, "pose feature", 1.0, "bjrc->bjrc", (R[:, first:first + 15], 1.0), add=(-eye.expand(B, 15, 3, 3),)).reshape(B, 135)
    vp = _stage(exact, "v_posed", 1 / 64, "bp,po->bo", (pf, 1.0), (pd, 1 / 64), add=(vs.reshape(B, 3 * V),)).reshape(B, V, 3)
    if fault == "one range unposed":
        lo, hi = mano_ranges(V)[MANO_UNPOSED_RANGE]
        vp[:, lo:hi] = vs[:, lo:hi]
    J = _stage(exact, "J", 1 / 512, "jv,bvc->bjc", (jr, 1 / 8), (vp if fault == "joints from v_posed" else vs, 1 / 64))
    GR, Gt = [None] * 16, [None] * 16
    for j in range(16):
        par = parents[j]
        if par < 0:
            GR[j], Gt[j] = R[:, j], J[:, j]
            continue
        pR, pt = (eye.expand(B, 3, 3), torch.zeros(B, 3, dtype=torch.float64)) if fault == "child before parent" else (GR[par], Gt[par])
        rel = _stage(exact, "J - J[parent]", 1 / 512, "bc->bc", (J[:, j], 1 / 512), add=(-J[:, par],))
        GR[j] = _stage(exact, "chain rotation", 1.0, "bik,bkc->bic", (pR, 1.0), (R[:, j], 1.0))
        Gt[j] = _stage(exact, "chain translation", 1 / 512, "bik,bk->bi", (pR, 1.0), (rel, 1 / 512), add=(pt,))
    GR, Gt = torch.stack(GR, 1), torch.stack(Gt, 1)
    At = Gt if fault == "A without G J" else _stage(exact, "A", 1 / 512, "bjik,bjk->bji", (GR, 1.0), (-J, 1 / 512), add=(Gt,))
    A = torch.cat([GR, At[..., None]], -1).reshape(B, 16, 12)
    T = _stage(exact, "blended transform", 1 / 2048, "vj,bje->bve", (w, 1 / 4), (A, 1 / 512)).reshape(B, V, 3, 4)
    verts = _stage(exact, "skinned vertex", 1 / 2048, "bvik,bvk->bvi", (T[..., :3], 1 / 4), (vp, 1 / 64), add=(T[..., 3],))
    tips = torch.tensor(synth.MANO_TIP_VERTS) - (1 if fault == "tips off by one" else 0)
    jmap = torch.tensor(synth.MANO_JOINT_MAP)
    if fault == "joint map rotated":
        jmap = jmap.roll(1)
    joints = torch.cat([Gt, verts[:, tips]], 1)[:, jmap]
    if exact:
        for t in (R, verts, joints):
            assert torch.equal(t.float().double(), t)
    f32 = np.float32
    c = cam.numpy().astype(f32)
    if fault == "cam columns rotated":
        c = c[:, [1, 2, 0]]
    jn = joints.float().numpy()
    with np.errstate(over="ignore"):
        tz = (f32(2.0) * f32(focal)) / (f32(image_size) * c[:, 0] + f32(1e-9))
    if exact:
        den = f32(image_size) * c[:, 0]
        live = c[:, 0] != 0
        assert np.array_equal((den + f32(1e-9))[live], den[live]), "the + 1e-9f is not absorbed"
        tz64 = 2.0 * focal / den[live].astype(np.float64)
        assert np.array_equal(tz64.astype(f32).astype(np.float64), tz64) and np.array_equal(tz[live].astype(np.float64), tz64), "tz is rounded"
    cam_t = np.stack([c[:, 1], c[:, 2], tz], 1)
    pz = jn[:, :, 2] + tz[:, None]
    f = f32(focal) / f32(image_size)
    kp2d = np.stack([((jn[:, :, 0] + c[:, 1:2]) / pz) * f, ((jn[:, :, 1] + c[:, 2:3]) / pz) * f], -1)
    assert cam_t.dtype == f32 and kp2d.dtype == f32
    return {"rotmats": R.float(), "verts": verts.float(), "joints": joints.float(), "cam_t": torch.from_numpy(cam_t), "kp2d": torch.from_numpy(kp2d)}


# ------------------------------------------------------------------------------------------------ Detect decode
# csrc/yolo.hip decode_kernel: pred row row0 + (a ny + y) nx + x, column c = f(sigmoid(raw[(y nx + x) ldraw + a no + c])).
# Exact data: every logit is a hashed choice among 0, +128 and -128; in fp32 expf(128) = +inf and expf(-128) = 0 (no fast-math),
# so the sigmoid 1 / (1 + expf(-r)) is exactly 1/2, 1 or 0, and with integer anchors and power-of-two strides
# xy = (2 s - 1/2 + grid) stride and wh = (2 s)^2 anchor are exact.
DECODE_GRIDS = [(1, 1), (3, 4), (5, 7), (17, 19)]        # (ny, nx); the last: 969 rows, three full workgroups and a partial one
DECODE_NC = [1, 3, 80]
DECODE_ROW0 = [0, 17]
DECODE_NB = [1, 3]
DECODE_PAD = [0, 8]                                      # ldraw = 3 no + pad, NaN in the padding columns
DECODE_TAIL_ROWS = 5                                     # rows of an image's slab after the last row written
DECODE_SENTINEL = -54321.0
DECODE_FAULTS = ["x and y grid swapped", "anchor w and h swapped", "anchor by p % 3", "-1/2 dropped", "rows in (y, x, a) order",
                 "row0 ignored", "raw as [c][a]", "raw image stride zero", "pred image stride zero"]
# Goes into every seed of the three-valued logits.  The (1, 1) grid has three rows and nc = 1 six columns each; a fault must
# change more than half of them at every shape (tests/test_exact_data_host.py), and this is the first salt under which it does.
DECODE_SALT = 2


def decode_cases():
    """Every (nb, ny, nx, nc, ldraw, row0, rows per image, level) of the exact GPU test; the anchor level cycles so that every grid
    meets all three."""
    out = []
    for nb in DECODE_NB:
        for gi, (ny, nx) in enumerate(DECODE_GRIDS):
            for ci, nc in enumerate(DECODE_NC):
                for pad in DECODE_PAD:
                    for row0 in DECODE_ROW0:
                        out.append((nb, ny, nx, nc, 3 * (5 + nc) + pad, row0, row0 + 3 * ny * nx + DECODE_TAIL_ROWS, (gi + ci + len(out)) % 3))
    return out


def decode_level(level):
    from hamer_yolo_amd.yolo import arch
    return float(arch.STRIDES[level]), [float(v) for v in arch.ANCHORS[level]]


def sigmoid_f32(raw):
    """1 / (1 + exp(-r)) in numpy.float32, one correctly rounded operation after the other (exp overflows to +inf on purpose)."""
    r = raw.numpy().astype(np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        return torch.from_numpy(np.float32(1.0) / (np.float32(1.0) + np.exp(-r)))


def decode_exact_case(nb, ny, nx, nc, ldraw, row0, stride_rows, seed=0):
    """raw (nb, ny nx, ldraw) fp32: 0, +128 or -128 by a hash of the flat index in the 3 no columns read, NaN in the padding.
    The three are equally likely but in the w and h columns, where -128 (a sigmoid of 0 and a box of size 0 whatever the
    anchor) is one in eight, so that nearly every row tells the anchors apart."""
    no = 5 + nc
    assert ldraw >= 3 * no and stride_rows >= row0 + 3 * ny * nx
    sd = _shape_seed(nb, ny, nx, nc, ldraw, row0, seed, DECODE_SALT)
    h = ints("exact.decode.raw", (nb, ny * nx, ldraw), 0, 23, sd).long()
    col = torch.arange(ldraw) % no
    wh = ((col == 2) | (col == 3)) & (torch.arange(ldraw) < 3 * no)
    pick = torch.where(wh[None, None, :], torch.where(h % 8 == 0, 2, (h // 8) % 2), h % 3)
    raw = torch.tensor([0.0, 128.0, -128.0])[pick]
    raw[:, :, 3 * no:] = float("nan")
    return raw


def decode_rule(s, ny, nx, nc, row0, stride_rows, level, fault=None, exact=True):
    """Detect's decode (yolo.py:148-184) in float64 on the sigmoids s (nb, ny nx, ldraw) of the raw logits -> pred
    (nb, stride_rows, no) float64, DECODE_SENTINEL in every row that is not written.  Row row0 + (a ny + y) nx + x takes
    s[p ldraw + a no + c], p = y nx + x: xy = (2 s - 1/2 + (x, y)) stride, wh = (2 s)^2 anchor_a, the rest s.
    `exact`: every value is an fp32 value (and, being a short dyadic number, is reached without a rounding)."""
    assert fault is None or fault in DECODE_FAULTS
    stride, anch = decode_level(level)
    nb, n, no = s.shape[0], ny * nx, 5 + nc
    s = s.double()
    a, p, c = torch.meshgrid(torch.arange(3), torch.arange(n), torch.arange(no), indexing="ij")
    y, x = p // nx, p % nx
    col = c * 3 + a if fault == "raw as [c][a]" else a * no + c
    img = torch.zeros(nb, dtype=torch.int64) if fault == "raw image stride zero" else torch.arange(nb)
    sv = s[img[:, None, None, None], p[None], col[None]]                      # (nb, 3, n, no)
    if fault == "x and y grid swapped":
        x, y = y, x
    aa = p % 3 if fault == "anchor by p % 3" else a
    aw, ah = torch.tensor(anch[0::2], dtype=torch.float64)[aa], torch.tensor(anch[1::2], dtype=torch.float64)[aa]
    if fault == "anchor w and h swapped":
        aw, ah = ah, aw
    half = 0.0 if fault == "-1/2 dropped" else 0.5
    v = torch.where(c == 0, (sv * 2 - half + x) * stride, torch.where(c == 1, (sv * 2 - half + y) * stride,
                    torch.where(c == 2, (sv * 2) ** 2 * aw, torch.where(c == 3, (sv * 2) ** 2 * ah, sv))))
    r0 = 0 if fault == "row0 ignored" else row0
    row = (r0 + p * 3 + a if fault == "rows in (y, x, a) order" else r0 + a * n + p)[:, :, 0]
    pred = torch.full((nb, stride_rows, no), DECODE_SENTINEL, dtype=torch.float64)
    for b in range(nb):
        pred[0 if fault == "pred image stride zero" else b, row] = v[b]
    if exact:
        assert torch.equal(pred.float().double(), pred) and torch.equal(pred * 4, (pred * 4).round()) and float(pred.abs().max()) * 4 < EXACT_LIMIT
    return pred


# General logits: hashed over +-8 on the 2^-23 grid, one in 32 replaced by +-30 or +-100.  The reference of the closeness test
# is the same formula in float64 and the bound is in fp32 ulps of the float64 value: twice the largest error of torch's CPU fp32
# evaluation of the formula on these very inputs, plus 2 ulp for a different expf -- taken per group of columns (xy, wh, and
# confidence with the classes), each of which is at most the one bound over all columns.  In the x and y columns a logit within
# DECODE_XY_CLEAR of -ln 3 is moved up by 1: there the sigmoid is 1/4, 2 s - 1/2 crosses zero in grid cell 0 and an ulp of the
# value measures the cancellation, not the arithmetic (unmoved, the CPU evaluation itself is 577 ulp off at one such element).
DECODE_GENERAL = [(3, 17, 19, 3, 3 * 8 + 8, 17, 0), (3, 17, 19, 80, 3 * 85, 0, 1), (1, 5, 7, 1, 3 * 6, 0, 2)]     # nb, ny, nx, nc, ldraw, row0, level
DECODE_XY_CLEAR = 0.5
DECODE_GROUPS = {"xy": slice(0, 2), "wh": slice(2, 4), "conf": slice(4, None)}
# Measured by tests/test_exact_data_host.py::test_decode_general_bound_is_the_measured_one, which fails if the CPU evaluation
# exceeds a value or stays below half of it.  The 26.6 of the confidences is one logit of -100: 1 / (1 + e^100) = 3.7e-44 is 26.5
# steps of 2^-149 and fp32 gives 0, its expf(100) being +inf.
DECODE_CPU_ULP = {"xy": 3.7, "wh": 3.6, "conf": 26.6}
DECODE_ULP_BOUND = {k: 2 * v + 2 for k, v in DECODE_CPU_ULP.items()}


def decode_general_case(nb, ny, nx, nc, ldraw):
    sd = _shape_seed(nb, ny, nx, nc, ldraw)
    raw = synth.uniform("decode.general.raw", (nb, ny * nx, ldraw), 8.0, seed=sd)
    col = torch.arange(ldraw) % (5 + nc)
    near = ((raw + float(np.log(3.0))).abs() < DECODE_XY_CLEAR) & (col < 2)[None, None, :]
    raw = torch.where(near, raw + 1.0, raw)
    big = torch.tensor([30.0, -30.0, 100.0, -100.0])[ints("decode.general.big", raw.shape, 0, 3, sd).long()]
    raw = torch.where(ints("decode.general.at", raw.shape, 0, 31, sd) == 0, big, raw)
    raw[:, :, 3 * (5 + nc):] = float("nan")
    return raw


def decode_f32_cpu(raw, ny, nx, nc, level):
    """torch's CPU fp32 evaluation of the kernel's formula, operation for operation -> the written rows (nb, 3 ny nx, no) fp32."""
    stride, anch = decode_level(level)
    nb, n, no = raw.shape[0], ny * nx, 5 + nc
    assert raw.dtype == torch.float32
    s = (1.0 / (1.0 + torch.exp(-raw[:, :, :3 * no]))).reshape(nb, n, 3, no).permute(0, 2, 1, 3)
    p = torch.arange(n)
    x, y = (p % nx).float()[None, None, :], (p // nx).float()[None, None, :]
    aw, ah = torch.tensor(anch[0::2])[None, :, None], torch.tensor(anch[1::2])[None, :, None]
    v = s.clone()
    v[..., 0], v[..., 1] = (s[..., 0] * 2.0 - 0.5 + x) * stride, (s[..., 1] * 2.0 - 0.5 + y) * stride
    t2, t3 = s[..., 2] * 2.0, s[..., 3] * 2.0
    v[..., 2], v[..., 3] = (t2 * t2) * aw, (t3 * t3) * ah
    assert v.dtype == torch.float32
    return v.reshape(nb, 3 * n, no)


def ulp32(v):
    """The spacing of fp32 at the float64 value v: 2^(floor(log2 |v|) - 23), 2^-149 below the normal range."""
    e = torch.frexp(v.double().abs())[1].double() - 1
    e = torch.where(v == 0, torch.full_like(e, -126.0), e)
    return torch.exp2(e.clamp_min(-126.0) - 23)


def ulp_error(got, ref):
    """max |got - ref| / ulp32(ref) over finite ref."""
    return float(((got.double() - ref.double()).abs() / ulp32(ref)).max())


# ------------------------------------------------------------------------------------------------ RootNet layout kernels
# hm_gap_linear: depth[b] = (sum_c mean_p feat[b, p, c] w[c] + bias) k_value[b].  Features -3..3, w -4..4, an integer bias, HW a
# power of two and k_value a multiple of 1/4: every column sum is an integer, s / HW and every product a multiple of 1 / HW.
GAP_C = [8, 200, 256, 264, 1024, 2048]     # < 256 leaves waves with nothing; 200 and 264 a partial 256-channel sweep
GAP_HW = [16, 64]
GAP_B = [1, 3]
GAP_SENTINEL = -777.0
GAP_FAULTS = ["feature as [C][HW]", "w rotated", "k_value rotated", "image stride zero"]
GAP_CLOSE = (3, 49, 2048)                  # (B, HW, C) of the closeness case
NHWC8_SHAPES = [(1, 1, 1), (1, 5, 7), (3, 16, 17), (2, 33, 31)]      # B HW = 1, 35, 816, 2046: below, and across multiples of 256
# (img_h, img_w_full, x0, win_w, patch, pad) of hm_patch_im2col: the full width without padding; the production window; a window
# that ends at the image's right edge (its padding is zero, not the neighbour's pixels); patch 8 in a non-square image; a narrow one
IM2COL_CASES = [(256, 256, 0, 256, 16, 0), (256, 256, 32, 192, 16, 2), (256, 256, 64, 192, 16, 2), (48, 80, 8, 40, 8, 3), (40, 24, 0, 24, 8, 0)]
IM2COL_B = [1, 3]
IM2COL_OUTSIDE = 32768.0                   # the pixels outside the window (an fp16 and bf16 value)


def gap_case(B, HW, C):
    """feat (B, HW, C) -3..3, w (C,) -4..4, bias (an integer), k_value (B,) distinct multiples of 1/4 in 1/4..3, all fp32, and
    depth (B,) fp32.  Asserts sum |s| |w| + HW |bias| < 2^24 in units of 1 / HW and that the final product is an fp32 value."""
    assert HW & (HW - 1) == 0
    sd = _shape_seed(B, HW, C)
    feat = ints("exact.gap.feat", (B, HW, C), -3, 3, sd)
    w = ints("exact.gap.w", (C,), -4, 4, sd)
    bias = float(ints("exact.gap.bias", (1,), -9, 9, sd))
    kv = ((int(ints("exact.gap.k", (1,), 0, 11, sd)) + torch.arange(B)) % 12 + 1).float() / 4
    return feat, w, bias, kv, gap_rule(feat, w, bias, kv)


def gap_rule(feat, w, bias, kv, fault=None, exact=True):
    """int64 column sums, one float64 quotient by HW (a power of two) -> depth (B,) fp32."""
    assert fault is None or fault in GAP_FAULTS
    B, HW, C = feat.shape
    f = feat.long()
    if fault == "feature as [C][HW]":
        f = f.reshape(B, C, HW).transpose(1, 2)
    if fault == "image stride zero":
        f = f[:1].expand(B, HW, C)
    wl = w.long().roll(1) if fault == "w rotated" else w.long()
    k = kv.roll(1) if fault == "k_value rotated" else kv
    s = f.sum(1)                                                                   # (B, C)
    num = (s * wl).sum(1)
    if exact:
        assert int(((s.abs() * wl.abs()).sum(1)).max()) + HW * abs(bias) < EXACT_LIMIT
    depth = (num.double() / HW + bias) * k.double()
    assert not exact or torch.equal(depth.float().double(), depth)
    return depth.float()


def nhwc8_case(B, H, W):
    """x (B, 3, H, W) fp32: hashed multiples of 1/16 in -8..8, values of fp32, fp16 and bf16 alike."""
    x = ints("exact.nhwc8.x", (B, 3, H, W), -127, 127, _shape_seed(B, H, W)) / 16
    assert torch.equal(x.half().float(), x) and torch.equal(x.bfloat16().float(), x)
    return x


def im2col_case(B, img_h, img_w_full, x0, win_w, patch, pad):
    """img (B, 3, img_h, img_w_full) fp32 on the 2^-23 grid of [-2, 2), IM2COL_OUTSIDE in every column outside the window."""
    img = synth.uniform("exact.im2col.img", (B, 3, img_h, img_w_full), 2.0, seed=_shape_seed(img_h, img_w_full, x0, win_w, patch, pad))
    img[..., :x0] = IM2COL_OUTSIDE
    img[..., x0 + win_w:] = IM2COL_OUTSIDE
    return img


def im2col_rule(img, x0, win_w, patch, pad, dtype):
    """F.unfold of the window rounded to `dtype` -> (B gh gw, 3 patch patch) fp32."""
    win = img[..., x0:x0 + win_w].to(dtype).float()
    ref = torch.nn.functional.unfold(win, kernel_size=patch, stride=patch, padding=pad)
    return ref.transpose(1, 2).reshape(-1, 3 * patch * patch)


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


# ------------------------------------------------------------------------------------------------ attention
# Code-book data whose softmax is exactly few-hot.  Per (crop, head) the keys are cut by a hashed permutation into groups of
# 1, 2 or 4; group g has a hashed sign code u_g in {-1, +1}^80, every key of the group is 8 u_g and every query is 8 u_g of the
# group of ONE key it is dealt by a second hashed permutation (so every key index is some query's chosen key).  q.k is 5120 on
# the query's own group and 64 (u_g . u_h) elsewhere; with the log2-domain scale 2^-3 the top scores are all exactly 640, the
# exponent of the chosen keys is exactly 0 and every other key lies at least ATT_GAP log2 units below, where an fp32 exponential
# is exactly zero (2^-149 is the smallest fp32 subnormal).  P is then 1 on the m keys of the group, the row sum m, 1 / m exact,
# and the accumulator the integer-valued sum of the group's V rows: the output is one rounding of an exactly known number.
ATT_T, ATT_HD, ATT_HDP = 192, 80, 96
ATT_LOG2E = np.float32(1.44269504088896340736)        # the constant launch_att multiplies the scale by, as fp32
ATT_C = 2.0 ** -3                                     # the log2-domain scale every exact case runs at
ATT_SCALE_DENSE = float(np.float32(ATT_C / 1.44269504088896340736))      # * ATT_LOG2E in fp32 is exactly 2^-3 (asserted in the tests)
ATT_SCALE_F32 = ATT_C                                 # attention_f32_kernel scales q first and uses expf
ATT_GAP = 160.0
# Goes into every seed, as LN_SALT does: the first salt under which every listed case meets the builder's assertions (gap,
# coverage of every key and query tile, scale-byte variety) and the fault fractions of tests/test_exact_data_host.py.
ATT_SALT = 0
ATT_DENSE = [(3, 4, (1,)), (3, 4, (1, 2, 4)), (2, 16, (1,)), (2, 16, (1, 2, 4))]      # (B, heads, group sizes): dense and MX8
ATT_F32 = [(1, 2, (1,)), (1, 2, (1, 2, 4)), (3, 4, (1,)), (3, 4, (1, 2, 4))]
ATT_PRODUCTION = (3, 4, (1,))                         # the dominant-key case run at scale 80^-0.5
ATT_TOME_B, ATT_TOME_HEADS = 3, 4
ATT_TOME_EDGES = [1, 15, 16, 17, 191, 192]
ATT_TOME_DECIDES = 192                                # tokens of the case in which the sizes decide (a multiple of 3)
ATT_SIZE_MAX = 8                                      # hashed sizes 1..8: log2 <= 3


def att_tome_tokens():
    """Every token count the attention of a block sees under the merging schedule of synth.HamerConfig() (r = (8, -1), the
    schedule HamerEngine(token_merge=True) runs), plus the edges."""
    from hamer_yolo_amd.engine import parse_tome_r
    t, seen = ATT_T, set(ATT_TOME_EDGES)
    for r in parse_tome_r(synth.HamerConfig().vit.depth, (8, -1)):
        seen.add(t)
        t -= min(r, t // 2)
    return sorted(seen)


def _hashed_perm(tag, shape, seed):
    """A hashed permutation of range(shape[-1]) for every leading index."""
    n = 1
    for s in shape:
        n *= int(s)
    h = synth._hash_u32(torch.arange(n, dtype=torch.int64), synth.name_seed(tag, seed)).reshape(*shape)
    return torch.argsort(h, dim=-1, stable=True)


def attention_case(B, heads, tokens, group_sizes, sizes=None):
    """q, k, v of the few-hot attention described above for B crops of `tokens` tokens.
    sizes: None; "hashed" (token sizes 1..ATT_SIZE_MAX, which shift a logit by at most 3 and leave P unchanged on dominant-key
    data); "decides" (group_sizes must be (3,): three identical keys with sizes 1, 1 and 2 in a hashed order, so the weights
    are 1/4, 1/4, 1/2 -- the partition is then shared by a crop's heads, as the sizes are).
    Returns a dict: qkv (B*tokens, 3*heads*80) fp32 (every value exact in bf16 and fp16), size (B*tokens,) fp32 or None,
    weights (B, heads, tokens, tokens) fp64 (the exact P / row sum), expect (B*tokens, heads*80) fp64 (weights @ V, exact),
    gap (the smallest distance in log2 units at scale 2^-3 between a chosen and any other logit, sizes included),
    chosen (B, heads, tokens) the key each query was dealt."""
    T, HD = int(tokens), ATT_HD
    assert 1 <= T <= ATT_T and all(m in (1, 2, 3, 4) for m in group_sizes)
    decides = sizes == "decides"
    assert not decides or (tuple(group_sizes) == (3,) and T % 3 == 0)
    assert decides or all(m in (1, 2, 4) for m in group_sizes)
    sd = _shape_seed(B, heads, T, len(group_sizes), sum(group_sizes), ATT_SALT)
    ph = 1 if decides else heads
    # partition: positions of a hashed permutation cut into runs whose lengths are hashed draws from group_sizes
    perm = _hashed_perm("exact.att.perm", (B, ph, T), sd)                                     # position -> key
    gs = torch.tensor(group_sizes, dtype=torch.int64)
    draw = gs[ints("exact.att.draw", (B, ph, T), 0, len(group_sizes) - 1, sd).long()]
    ends = draw.cumsum(-1)
    pos = torch.arange(T, dtype=torch.int64).expand(B, ph, T).contiguous()
    gpos = torch.searchsorted(ends, pos, right=True)                                          # group of a position
    # a clipped last run whose length is no legal group size (3 of a drawn 4) becomes single keys
    start = torch.where(gpos > 0, torch.gather(ends, -1, (gpos - 1).clamp(min=0)), torch.zeros_like(gpos))
    last = gpos[..., -1:]
    clipped = T - torch.gather(start, -1, torch.full_like(last, T - 1))
    legal = (clipped[..., None] == gs).any(-1)
    gpos = torch.where((gpos == last) & ~legal, last + (pos - start), gpos)
    group = torch.empty_like(gpos).scatter_(-1, perm, gpos).expand(B, heads, T)               # key -> group
    member = torch.empty_like(gpos).scatter_(-1, perm, pos - start).expand(B, heads, T)       # key -> place inside its group
    counts = torch.zeros(B, heads, 2 * T, dtype=torch.int64).scatter_add_(-1, group, torch.ones_like(group))
    assert all(int(c) in tuple(group_sizes) + (0,) or int(c) == 1 for c in counts.unique())
    # codes, keys, queries
    u = 2 * ints("exact.att.code", (B, heads, 2 * T, HD), 0, 1, sd) - 1
    k = 8 * torch.gather(u, 2, group[..., None].expand(B, heads, T, HD))
    chosen = _hashed_perm("exact.att.deal", (B, heads, T), sd)                                # query -> the key it is dealt
    qgroup = torch.gather(group, -1, chosen)
    q = 8 * torch.gather(u, 2, qgroup[..., None].expand(B, heads, T, HD))
    # V: ints(-7..7) * 2^e, e hashed per (crop, token, head, 32-column block)
    e = ints("exact.att.vexp", (B, T, heads, 3), 0, 4, sd).to(torch.int32).repeat_interleave(32, dim=-1)[..., :HD]
    v = torch.ldexp(ints("exact.att.v", (B, T, heads, HD), -7, 7, sd), e).permute(0, 2, 1, 3)
    size = lsz = None
    if sizes == "hashed":
        size = 1.0 + ints("exact.att.size", (B, T), 0, ATT_SIZE_MAX - 1, sd)
    elif decides:
        big = ints("exact.att.big", (B, 1, 2 * T), 0, 2, sd).long()                          # which of the three keys carries size 2
        size = 1.0 + (member[:, :1] == torch.gather(big, -1, group[:, :1])).float()[:, 0]
    else:
        assert sizes is None
    if size is not None:
        lsz = size.double().log2()
    # the exact P: own group, weighted by size where the sizes decide (the hashed sizes act on single keys and cancel)
    own = (qgroup[..., :, None] == group[..., None, :]).double()
    w = own * (size.double()[:, None, None, :] if decides else 1.0)
    rowsum = w.sum(-1, keepdim=True)
    assert all(float(r) in (1.0, 2.0, 4.0) for r in rowsum.unique())
    weights = w / rowsum
    expect = weights @ v.double()
    # the gap: chosen logits against the rest, in log2 units at scale 2^-3
    z = (q.double() @ k.double().transpose(-1, -2)) * ATT_C
    assert bool((z[own.bool()] == 5120 * ATT_C).all())
    if lsz is not None:
        z = z + lsz[:, None, None, :]
    top = torch.where(own.bool(), z, torch.full_like(z, float("inf"))).amin(-1)
    rest = torch.where(own.bool(), torch.full_like(z, -float("inf")), z).amax(-1)
    gap = float((top - rest).min()) if bool((~own.bool()).any()) else float("inf")
    assert gap >= ATT_GAP, ((B, heads, T, group_sizes, sizes), gap)
    if sizes == "hashed":
        assert all(m == 1 for m in group_sizes), "hashed sizes leave P unchanged on dominant-key data only"
    # coverage: every key is some query's chosen key, every query tile is there by construction (all T queries run)
    hit = torch.zeros(B, heads, T, dtype=torch.int64).scatter_add_(-1, chosen, torch.ones_like(chosen))
    assert bool((hit >= 1).all()), "a key index is nobody's chosen key"
    qkv = torch.stack([q, k, v], 0).permute(1, 3, 0, 2, 4).reshape(B * T, 3 * heads * HD).contiguous()
    for dt in (torch.bfloat16, torch.float16):
        assert torch.equal(qkv.to(dt).float(), qkv)
    assert torch.equal((expect * 4).round(), expect * 4) and float(expect.abs().max()) <= 7 * 16
    return {"qkv": qkv, "size": None if size is None else size.reshape(B * T).contiguous(), "weights": weights,
            "expect": expect.permute(0, 2, 1, 3).reshape(B * T, heads * HD).contiguous(), "gap": gap, "chosen": chosen,
            "group": group, "q": q.double(), "k": k.double(), "v": v.double(), "log2size": lsz}


def att_mx8_expect(expect, heads):
    """(bytes (rows, heads*96), scales (heads*3, rows)) of the oracle quantiser on the exact fp32 rows, every head widened to
    96 columns with zeros."""
    from oracle import fp8_ref as Q
    rows = expect.shape[0]
    f = expect.float()
    assert torch.equal(f.double(), expect)
    pad = torch.zeros(rows, heads, ATT_HDP)
    pad[:, :, :ATT_HD] = f.reshape(rows, heads, ATT_HD)
    q8, sc = Q.mx8_quantize(pad.reshape(rows, heads * ATT_HDP))
    assert bool((q8.reshape(rows, heads, ATT_HDP)[:, :, ATT_HD:] == 0).all())
    return q8, sc


def att_production_margin(case, scale, dtype):
    """The dominant-key case at an ordinary scale: fma(m, c, -(m c)) is the rounding residual of m c, so p = exp2(residual)
    is within about 1e-5 of 1 and the output v / p.  Emulates the two roundings (p to the operand type, which must give 1;
    v / p to the output type, which must give v back for every V value in use, with the hardware exponential allowed an
    error of 2^-21 relative on top) and returns (c, residual, delta)."""
    c = np.float32(scale) * ATT_LOG2E
    assert c.dtype == np.float32
    m = np.float32(5120.0)
    mneg = -(m * c)                                                       # fp32 product, rounded
    res = float(np.float32(float(m) * float(c) + float(mneg)))            # the fma: exact in fp64, then one rounding
    delta = abs(2.0 ** res - 1.0) + 2.0 ** -21
    one = torch.tensor([1.0 + delta, 1.0 - delta], dtype=torch.float64)
    assert torch.equal(one.float().to(dtype).double(), torch.ones(2, dtype=torch.float64)), "P would not round to 1"
    vals = case["v"].unique()
    for f in (1.0 / (1.0 + delta), 1.0 / (1.0 - delta)):
        assert torch.equal((vals * f).float().to(dtype).double(), vals), "v / p would not round back to v"
    # every other key still underflows: the gap at this scale
    assert case["gap"] / ATT_C * float(c) - 1.0 >= ATT_GAP
    return float(c), res, delta
