"""hm_gemm_fp8 -- the one-tile kernel (gemm_fp8_kernel) and the persistent one (gemm_fp8p_kernel) -- with its three epilogues on
exact data (tests/exact_data.py: fp8_epilogue_case).

Operands are hashed integers that e4m3 holds exactly and hashed power-of-two scales, so every product and sum is exact in fp32:
RESID_F32 must equal acc + bias + resid, STORE the same sum without the residual rounded ONCE to bf16, and GELU_MX8 the oracle
quantiser applied to max(v, 0) -- its bias puts every |v| at or above 16, where both GELU implementations (gelu_fast2 here,
F.gelu in the oracle) are exactly max(v, 0), and makes the block maxima straddle 448 2^k, so the output scale bytes depend on the
row and on the block and about a fifth of the blocks are all zero.  Every comparison is torch.equal; for the e4m3 bytes the sign
of a zero byte is masked on both sides (the kernel gives +0 where torch gives -0), nothing else.
tests/test_exact_data_host.py shows which faults this data sees.

Which kernel a call takes is asked of the library for the very arguments of the call: hm_gemm_fp8_persistent, the function
hm_gemm_fp8 itself dispatches on (whole 256 x 256 tiles, at least 8 of them, K >= 256, a bias, HM_OPT_FP8_ONE_TILE unset;
RESID_F32 also needs HM_OPT_FP8P_RESID, and GELU_MX8 ldc % 16 == 0), and asserted before every launch.  Outputs are written
into sentinel-filled buffers with pad columns and a spare row.
"""
import ctypes as C
import functools
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exact_data as ED  # noqa: E402

from hamer_yolo_amd import lib as L

DEV = "cuda"
EPIS = {"store": L.HM_EPI_STORE, "resid": L.HM_EPI_RESID_F32, "gelu": L.HM_EPI_GELU_MX8}
PAD_BYTE = 0x7F                                   # the e4m3 NaN: an operand read past K would poison its sum


@functools.lru_cache(maxsize=None)
def _case(M, N, K):
    """Operands and the three expectations, built once per shape on the CPU and left unchanged."""
    c = ED.fp8_epilogue_case(M, N, K)
    acc, bias = c["acc"], c["bias"].double()
    c["expect"] = {"store": (acc + bias).float().to(torch.bfloat16), "resid": (acc + bias + c["resid"].double()).float(),
                   "gelu": ED.fp8_gelu_expect(acc + c["gelu_bias"].double()),
                   "store_nobias": acc.float().to(torch.bfloat16), "resid_nobias": (acc + c["resid"].double()).float()}
    return c


def _wide(t, ld, fill):
    """t (rows, cols) as a column slice of a (rows, ld) device buffer filled with `fill`."""
    buf = torch.full((t.shape[0], ld), fill, dtype=t.dtype, device=DEV)
    buf[:, :t.shape[1]] = t.to(DEV)
    return buf[:, :t.shape[1]]


def _run(c, M, N, K, epi, persistent, bias=True, ldx=None, ldw=None, ldc=None, ldr=None, inplace=False):
    """One call of hm_gemm_fp8 into sentinel-filled buffers, on the kernel `persistent` says (asserted from the library); returns the result on the CPU after checking that pad columns,
    the spare row and the guard behind the scales came back untouched."""
    x8 = _wide(c["x8"], ldx or K, PAD_BYTE)
    w8 = _wide(c["w8"], ldw or K, PAD_BYTE)
    xs, ws = c["xs"].to(DEV), c["ws"].to(DEV)
    b = (c["gelu_bias"] if epi == "gelu" else c["bias"]).to(DEV) if bias else None
    ldc = ldc or N
    resid = out_scales = flat = None
    if epi == "store":
        raw = torch.full((M + 1, ldc), -1, dtype=torch.int16, device=DEV)
        out = raw.view(torch.bfloat16)
    elif epi == "resid":
        raw = torch.full((M + 1, ldc), -1, dtype=torch.int32, device=DEV)
        out = raw.view(torch.float32)
        if inplace:
            assert ldr is None
            out[:M, :N] = c["resid"].to(DEV)
            resid = out
        else:
            resid = _wide(c["resid"], ldr or N, float("nan"))
    else:
        raw = torch.full((M + 1, ldc), 0xFF, dtype=torch.uint8, device=DEV)
        out = raw
        flat = torch.full(((N // 32) * M + 256,), 0xFF, dtype=torch.uint8, device=DEV)
        out_scales = flat[:(N // 32) * M].view(N // 32, M)
    a = L.GemmFp8Args(L.ptr(x8), L.ptr(xs), L.ptr(w8), L.ptr(ws), L.ptr(out), L.ptr(b), L.ptr(resid), L.ptr(out_scales), M, N, K,
                      x8.stride(0), w8.stride(0), ldc, resid.stride(0) if resid is not None else 0, EPIS[epi], L.HM_DTYPE_BF16)
    route = L.load().hm_gemm_fp8_persistent(C.byref(a))
    assert route == int(persistent), f"{epi} {(M, N, K)} ldc={ldc}: hm_gemm_fp8_persistent says {route}, the test expects {int(persistent)}"
    L.check(L.load().hm_gemm_fp8(C.byref(a), L.current_stream()), "hm_gemm_fp8")
    sentinel = 0xFF if epi == "gelu" else -1
    assert bool((raw[M:] == sentinel).all()) and bool((raw[:M, N:] == sentinel).all()), "pad columns or the spare row overwritten"
    if epi == "gelu":
        assert bool((flat[(N // 32) * M:] == 0xFF).all()), "bytes behind the scales overwritten"
        return out[:M, :N].cpu(), out_scales.cpu()
    return out[:M, :N].cpu()


def _check(c, got, epi, what, bias=True):
    exp = c["expect"][epi if bias else epi + "_nobias"]
    if epi == "gelu":
        ED.assert_exact(got[1], exp[1], f"{what}: scales")
        ED.assert_exact(ED.fp8_unsigned_zero(got[0]), ED.fp8_unsigned_zero(exp[0]), f"{what}: e4m3 bytes")
    elif epi == "store":
        ED.assert_exact(got.view(torch.int16), exp.view(torch.int16), what)
    else:
        ED.assert_exact(got, exp, what)


@pytest.mark.parametrize("M,N,K", ED.GEMM_FP8_ONE_TILE)
def test_one_tile_kernel_every_epilogue_exact(M, N, K):
    """gemm_fp8_kernel: the smallest legal problem (one K-step, every row and scale copy clamped), a last 16-row scale copy
    clamped to M - 16, ragged 3 x 3 tiles, 40 K-steps, 9 whole tiles.  HM_OPT_FP8_ONE_TILE keeps (768, 768, 1280) out of the
    persistent kernel.  RESID_F32 also in place."""
    c = _case(M, N, K)
    with L.option(L.HM_OPT_FP8_ONE_TILE, 1):
        for epi in EPIS:
            _check(c, _run(c, M, N, K, epi, False), epi, f"one-tile {epi} {(M, N, K)}")
        _check(c, _run(c, M, N, K, "resid", False, inplace=True), "resid", f"one-tile resid in place {(M, N, K)}")


@pytest.mark.parametrize("M,N,K,grids", ED.GEMM_FP8_PERSISTENT)
def test_persistent_kernel_every_epilogue_exact(M, N, K, grids):
    """gemm_fp8p_kernel, every call twice in a row: the minimum K (two steps) at the device's grid; on 8 workgroups 9 tiles of
    three K-steps (one workgroup takes two tiles, the ring slot parity flipped between them) and 20 tiles (XCD runs of 3 and
    2, odd step count); an even step count on 8 and 16 workgroups.  RESID_F32 (HM_OPT_FP8P_RESID) also in place."""
    c = _case(M, N, K)
    tiles = (M // 256) * (N // 256)
    for grid in grids:
        with L.option(L.HM_OPT_FP8P_GRID, grid), L.option(L.HM_OPT_FP8P_RESID, 1):
            print(f"{(M, N, K)}: {tiles} tiles of {K // 128} K-steps on {grid or 'one per CU or tile'} workgroups")
            for rep in range(2):
                for epi in EPIS:
                    _check(c, _run(c, M, N, K, epi, True), epi, f"persistent {epi} {(M, N, K)} grid {grid} run {rep}")
                _check(c, _run(c, M, N, K, "resid", True, inplace=True), "resid", f"persistent resid in place {(M, N, K)} grid {grid} run {rep}")


@pytest.mark.parametrize("M,N,K", ED.GEMM_FP8_NO_BIAS)
def test_null_bias_exact(M, N, K):
    """bias = NULL: STORE and RESID_F32 (GELU_MX8's exactness rests on its bias).  (512, 1024, 256) has 8 whole tiles but no
    bias, so it takes the one-tile kernel."""
    c = _case(M, N, K)
    with L.option(L.HM_OPT_FP8P_RESID, 1):
        for epi in ("store", "resid"):
            _check(c, _run(c, M, N, K, epi, False, bias=False), epi, f"{epi} without bias {(M, N, K)}", bias=False)


@pytest.mark.parametrize("M,N,K", ED.GEMM_FP8_WIDE)
def test_wide_leading_dimensions_exact(M, N, K):
    """x8 and w8 as column slices of wider buffers (ldx = K + 48, ldw = K + 32, the pad an e4m3 NaN); STORE and RESID_F32 with
    ldc = N + 8 and a residual of ldr = N + 4; GELU_MX8 with ldc = N + 16 (stays persistent at (768, 768, 384)) and with
    ldc = N + 8 (falls back to the one-tile kernel).  (768, 768, 384) runs on 8 workgroups."""
    c = _case(M, N, K)
    big = M % 256 == 0
    with L.option(L.HM_OPT_FP8P_GRID, 8 if big else 0), L.option(L.HM_OPT_FP8P_RESID, 1):
        for epi, ldc, ldr, persistent in (("store", N + 8, None, big), ("resid", N + 8, N + 4, big), ("gelu", N + 16, None, big),
                                          ("gelu", N + 8, None, False)):
            got = _run(c, M, N, K, epi, persistent, ldx=K + 48, ldw=K + 32, ldc=ldc, ldr=ldr)
            _check(c, got, epi, f"{epi} ldc={ldc} ldr={ldr} {(M, N, K)} ({'persistent' if persistent else 'one-tile'})")
