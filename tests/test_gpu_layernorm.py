"""Every kernel path of csrc/norm.hip, on data whose LayerNorm is exact (tests/exact_data.py, eps = 0.75: mean m_r, rstd 1,
y = sigma * gamma / 2 + beta in 5 significant bits) and on rows that make eps, the mean and the two-pass variance visible.

Which (M, D) selects which instantiation, with CUs the device's compute units (256 on MI355X) and mj = ceil(D / 256):

hm_layernorm -> launch_ln -> layernorm_rows_kernel<OutT, MAXJ>, OutT in float / bf16 / fp16 (all three run at every shape)
  MAXJ = 1  mj <= 1   D = 4, 96, 252 unpaired;  D = 256 "full" (one 8-byte store per lane: MAXJ is odd, no pair)
  MAXJ = 2  mj == 2   D = 260, 320 unpaired;    D = 512 full: one paired 16-byte store
  MAXJ = 4  mj 3, 4   D = 516, 768 unpaired;    D = 1024 full: two paired stores
  MAXJ = 5  mj == 5   D = 1028, 1276 unpaired;  D = 1280 full: two paired stores and the odd piece
  MAXJ = 8  mj 6..8   D = 1284, 1536, 2044 unpaired;  D = 2048 full: four paired stores
  "full" is D == MAXJ * 256 with a 16-bit OutT; float output always takes the unpaired 16-byte stores.
  rows per wave rpw = ceil(M / (16 CUs)): 1 at M = 1, 3, 5, 197 (the row loop runs once, nothing is prefetched);
  2 at M = 16 CUs + 1 (grid of 8 CUs + 1 waves rounded up to workgroups: most waves run two rows, the last ones one);
  3 at M = 32 CUs + 5 (ragged last round) and at M = 48 CUs (every wave three rows).  The large M run at
  D = 96, 256, 512, 1280, 2048: MAXJ 1 unpaired, and every full path.

hm_layernorm_accum -> launch_ln_acc -> layernorm_kernel<OutT, MAXJ, true>, one row per wave
  MAXJ = 2  mj <= 2   D = 4, 320, 512
  MAXJ = 5  mj 3..5   D = 1280
  MAXJ = 8  mj 6..8   D = 1284, 2048
  slab counts 1, 4, 5, 10 against the loop's unroll of 4: below, whole, one over, two rounds and a half.

hm_layernorm_mx8 -> layernorm_mx8_kernel<MAXJ>, one row per wave
  MAXJ = 2  mj <= 2   D = 32 (one 8-lane group), 64, 256, 288, 512
  MAXJ = 5  mj 3..5   D = 544, 1280
  MAXJ = 8  mj 6..8   D = 1312, 1536, 2048

Every exact test ends in torch.equal of whole tensors.  Output buffers are filled with NaN bytes before the call and carry one
spare row that must still hold them afterwards.  The faults this data sees are listed in tests/test_exact_data_host.py.

The accuracy test bounds |kernel - fp64| per row by 4 x the error of a plain torch fp32 two-pass LayerNorm on the same rows,
measured on the CPU in units of 2^-23 (max|x - mean| / sqrt(var + eps) max|gamma| + |mean| / sqrt(var + eps)):
uniform rows 1.52, mean 1000 0.95, mean -3000 0.80, variance = eps 1.69, variance = 1e-3 eps 2.28, one outlier of 1e4 1.86,
all-zero row 0 (ED.LN_MULTIPLES holds them rounded up: 1.6, 1.0, 0.9, 1.7, 2.3, 1.9, 0).  The factor 4 is for the kernels'
other reduction order.  test_exact_data_host.py feeds a one-pass variance and an eps outside or without the root through the
same bound: they miss it by more than 100 x.
"""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exact_data as ED  # noqa: E402

from hamer_yolo_amd import lib as L
from oracle import fp8_ref as Q

DEV = "cuda"
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
LARGE_M = ["16cus+1", "32cus+5", "48cus"]


def _code(dt):
    return {torch.float32: L.HM_OUT_F32, torch.bfloat16: L.HM_DTYPE_BF16, torch.float16: L.HM_DTYPE_F16}[dt]


def _poisoned(rows, cols, dt):
    """(rows + 1, cols) of 0xFF bytes (NaN in every float format here): the kernel gets the first `rows` rows."""
    size = torch.empty((), dtype=dt).element_size()
    return torch.full(((rows + 1) * cols * size,), 0xFF, dtype=torch.uint8, device=DEV).view(dt).view(rows + 1, cols)


def _spare_row_untouched(buf):
    return bool((buf[-1].contiguous().view(torch.uint8) == 0xFF).all())


def _layernorm(x, gamma, beta, eps, dt):
    M, D = x.shape
    buf = _poisoned(M, D, dt)
    L.check(L.load().hm_layernorm(L.ptr(x), L.ptr(gamma), L.ptr(beta), L.ptr(buf), _code(dt), M, D, eps, L.current_stream()), "hm_layernorm")
    assert _spare_row_untouched(buf), "hm_layernorm wrote past row M - 1"
    return buf[:M]


def _layernorm_accum(x, parts, bias, gamma, beta, eps, dt):
    M, D = x.shape
    buf = _poisoned(M, D, dt)
    L.check(L.load().hm_layernorm_accum(L.ptr(x), L.ptr(parts), parts.shape[0], L.ptr(bias), L.ptr(gamma), L.ptr(beta), L.ptr(buf),
                                        _code(dt), M, D, eps, L.current_stream()), "hm_layernorm_accum")
    assert _spare_row_untouched(buf), "hm_layernorm_accum wrote past row M - 1"
    return buf[:M]


def _layernorm_mx8(x, gamma, beta, eps):
    M, D = x.shape
    o8 = _poisoned(M, D, torch.uint8)
    sc = _poisoned(D // 32, M, torch.uint8)
    L.check(L.load().hm_layernorm_mx8(L.ptr(x), L.ptr(gamma), L.ptr(beta), L.ptr(o8), L.ptr(sc), M, D, eps, L.current_stream()),
            "hm_layernorm_mx8")
    assert _spare_row_untouched(o8) and _spare_row_untouched(sc), "hm_layernorm_mx8 wrote past its outputs"
    return o8[:M], sc[:D // 32]


def _equal(got, ref, what):
    """torch.equal on the device; the located report of ED.assert_exact only when it fails."""
    ref = ref.to(got.device)
    if not torch.equal(got, ref):
        ED.assert_exact(got, ref, what)
    assert torch.equal(got, ref), what


def _with_constant_row(x, beta, y):
    """From three rows up the middle row is constant: centred values and variance are 0, the output is beta bit for bit."""
    M = x.shape[0]
    if M >= 3:
        x, y = x.clone(), y.clone()
        x[M // 2] = 3.0
        y[M // 2] = beta.double()
    return x, y


def _ln_exact(M, D):
    x, gamma, beta, y = ED.ln_case(M, D)
    x, y = _with_constant_row(x, beta, y)
    xd, gd, bd, yd = x.to(DEV), gamma.to(DEV), beta.to(DEV), y.float().to(DEV)
    for dt in DTYPES:
        _equal(_layernorm(xd, gd, bd, ED.LN_EPS, dt), yd.to(dt), ("hm_layernorm", M, D, dt))


# ------------------------------------------------------------------------------------------------ exact
@pytest.mark.parametrize("M", ED.LN_M)
@pytest.mark.parametrize("D", ED.LN_D)
def test_layernorm_exact(D, M):
    """One row per wave, every width class on both store paths, three output types: equal to the closed form."""
    _ln_exact(M, D)


@pytest.mark.parametrize("which", range(3), ids=LARGE_M)
@pytest.mark.parametrize("D", ED.LN_LARGE_M_D)
def test_layernorm_exact_rows_per_wave(D, which):
    """The production row loop: 2, 3 (ragged last round) and 3 (whole) rows per wave, the next row prefetched under the
    current row's reductions, rows striding by the waves of the grid."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    M = ED.ln_large_m(cus)[which]
    assert -(-M // (16 * cus)) == (2, 3, 3)[which]
    _ln_exact(M, D)


@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("D", ED.LN_ACCUM_D)
def test_layernorm_accum_exact(D, bias):
    """x += bias + slabs in place equals the exact sum, the output the closed form, and a second call on fresh copies gives
    the same bytes; bias present and NULL, three output types, slab counts around the loop's unroll of 4."""
    for M in ED.LN_ACCUM_M:
        for S in ED.LN_ACCUM_S:
            x0, parts, b, x, gamma, beta, y = ED.ln_accum_case(M, D, S, bias)
            pd, bsd, gd, bd = parts.to(DEV), (b.to(DEV) if bias else None), gamma.to(DEV), beta.to(DEV)
            xsum, yd = x.to(DEV), y.float().to(DEV)
            for dt in DTYPES:
                what = ("hm_layernorm_accum", M, D, S, bias, dt)
                xa = x0.to(DEV).clone()
                out = _layernorm_accum(xa, pd, bsd, gd, bd, ED.LN_EPS, dt)
                _equal(xa, xsum, what + ("x",))
                _equal(out, yd.to(dt), what + ("out",))
                xb = x0.to(DEV).clone()
                out2 = _layernorm_accum(xb, pd.clone(), bsd, gd, bd, ED.LN_EPS, dt)
                assert torch.equal(xa, xb) and torch.equal(out.view(torch.uint8), out2.view(torch.uint8)), what


@pytest.mark.parametrize("M", ED.LN_MX8_M)
@pytest.mark.parametrize("D", ED.LN_MX8_D)
def test_layernorm_mx8_exact(D, M):
    """y is exact and the quantiser deterministic (ties to even on both sides): ALL value bytes and ALL scale bytes, laid out
    [D/32][M], equal the oracle quantiser's of the closed form."""
    x, gamma, beta, y = ED.ln_case(M, D)
    x, y = _with_constant_row(x, beta, y)
    r8, rs = Q.mx8_quantize(y.float())
    o8, sc = _layernorm_mx8(x.to(DEV), gamma.to(DEV), beta.to(DEV), ED.LN_EPS)
    _equal(sc, rs, ("hm_layernorm_mx8 scales", M, D))
    _equal(o8, r8, ("hm_layernorm_mx8 values", M, D))


# ------------------------------------------------------------------------------------------------ accuracy
@pytest.mark.parametrize("eps", ED.LN_HOSTILE_EPS)
@pytest.mark.parametrize("D", ED.LN_HOSTILE_D)
def test_layernorm_accuracy_on_hostile_rows(D, eps):
    """Against fp64 on uniform rows, rows of mean 1000 (unit spread) and -3000 (spread 0.1), rows whose variance is eps and
    1e-3 eps, rows with one outlier of 1e4, and all-zero rows (six of each, |x| <= 1e4).  fp32 output within
    4 x ED.LN_MULTIPLES x ED.ln_error_unit per row (the multiples are those of a torch fp32 two-pass LayerNorm, measured on the
    CPU: uniform 1.52, mean 1000 0.95, mean -3000 0.80, var = eps 1.69, var = 1e-3 eps 2.28, outlier 1.86, zero 0; see the
    module docstring), the 16-bit outputs within that plus one step of their format.  hm_layernorm_accum runs the same rows as
    one slab on top of zeros."""
    x, gamma, beta, kind = ED.ln_hostile_rows(D, eps)
    ref = ED.ln_reference(x, gamma, beta, eps)
    bound = ED.ln_error_bound(x, gamma, eps, kind)
    xd, gd, bd = x.to(DEV), gamma.to(DEV), beta.to(DEV)
    outs = [("hm_layernorm", dt, _layernorm(xd, gd, bd, eps, dt)) for dt in DTYPES]
    for dt in DTYPES:
        x0 = torch.zeros_like(xd)
        outs.append(("hm_layernorm_accum", dt, _layernorm_accum(x0, xd[None].clone(), None, gd, bd, eps, dt)))
        assert torch.equal(x0, xd)
    failed = []
    for name, dt, out in outs:
        err = (out.cpu().double() - ref).abs()
        allowed = bound if dt == torch.float32 else bound + ED.ulp16(ref, dt)
        for i, k in enumerate(ED.LN_HOSTILE_KINDS):
            rows = kind == i
            e, a = err[rows], allowed.expand_as(err)[rows]
            worst = float((e / a.clamp_min(1e-300)).max()) if k != "zero" or dt != torch.float32 else float(e.max())
            print(f"D {D} eps {eps} {name} {dt} {k}: max err {float(e.max()):.3e}, worst err / allowed {worst:.3f}")
        assert torch.isfinite(out).all()
        if not (err <= allowed).all():
            failed.append((name, dt))
    assert not failed, failed


# ------------------------------------------------------------------------------------------------ absmax16, broadcast_rows
def _absmax(x, col0, ncols, preload=0.0):
    slot = torch.full((1,), preload, dtype=torch.float32, device=DEV)
    code = L.HM_DTYPE_BF16 if x.dtype == torch.bfloat16 else L.HM_DTYPE_F16
    L.check(L.load().hm_absmax16(L.ptr(x), x.stride(0), x.shape[0], col0, ncols, code, L.ptr(slot), L.current_stream()), "hm_absmax16")
    return slot.cpu()[0]


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("M,ld,col0,ncols", [(1, 8, 0, 8), (197, 3840, 1280, 1280), (300, 100, 37, 3), (5000, 64, 0, 64)])
def test_absmax16(M, ld, col0, ncols, dt):
    """max|x| of a column window of a 16-bit matrix, folded into the slot by an atomic max: exact; the window is respected
    (a larger element sits just outside of it, on either side where there is one); the largest element may be the window's
    first, its last or one in the middle (past 1024 x 256 elements at M = 5000: the grid-stride loop's second round); a larger
    value already in the slot stays; inf and NaN read back non-finite from inside the window only."""
    from hamer_yolo_amd import synth
    base = synth.uniform("absmax", (M, ld), 0.9, seed=M + ld).to(dt)
    outside = [c for c in (col0 - 1, col0 + ncols) if 0 <= c < ld]
    spots = {"first": (0, col0), "last": (M - 1, col0 + ncols - 1), "middle": (M - 1 - M // 9, col0 + ncols // 2)}
    plain = base.to(DEV)
    assert float(_absmax(plain, col0, ncols)) == float(base[:, col0:col0 + ncols].abs().max()) < 1.0
    for name, (r, c) in spots.items():
        x = base.clone()
        x[r, c] = -3.0
        for oc in outside:
            x[r, oc] = 7.0
            x[M // 2, oc] = -7.0
        want = x[:, col0:col0 + ncols].abs().max().float()
        assert float(want) == 3.0
        xd = x.to(DEV)
        got = _absmax(xd, col0, ncols)
        assert float(got) == float(want), (name, float(got))
        assert float(_absmax(xd, col0, ncols, preload=10.0)) == 10.0, name
        assert float(_absmax(xd, col0, ncols, preload=1.5)) == 3.0, name
        for bad in (float("inf"), float("-inf"), float("nan")):
            xi = x.clone()
            xi[r, c] = bad
            assert not torch.isfinite(_absmax(xi.to(DEV), col0, ncols)), (name, bad)
            for oc in outside:
                xo = x.clone()
                xo[r, oc] = bad
                assert float(_absmax(xo.to(DEV), col0, ncols)) == 3.0, (name, bad, oc)


@pytest.mark.parametrize("B,D", [(1, 4), (5, 1024), (37, 1023)])
def test_broadcast_rows(B, D):
    vec = ED.ints("broadcast", (D,), -1000, 1000, D) / 8
    out, vd = _poisoned(B, D, torch.float32), vec.to(DEV)
    L.check(L.load().hm_broadcast_rows(L.ptr(vd), L.ptr(out), B, D, L.current_stream()), "hm_broadcast_rows")
    assert _spare_row_untouched(out)
    _equal(out[:B], vec.expand(B, D), ("hm_broadcast_rows", B, D))
