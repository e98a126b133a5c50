"""The staggered K loop of the two 256 x 256 GEMM kernels (HM_OPT_GEMM_STAGGER = 2: gemm_pxs_kernel, gemm_x3rs_kernel).

Waves 4-7 run one sub-step behind waves 0-3: they carry a fragment set across every barrier, multiply it first in the next
interval, and keep one MFMA run for behind the post-loop barrier.  Every wave's MFMA and fp32-add order is the lockstep
kernel's, so each test here ends in equal bytes: exact-integer data against torch, random data against option 1."""
import ctypes as C
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exact_data as ED  # noqa: E402

from hamer_yolo_amd import lib as L
from hamer_yolo_amd import ops, synth
from hamer_yolo_amd.engine import HamerEngine

DEV = "cuda"
LOCKSTEP, STAGGERED = 1, 2
PX_SHAPES = [(512, 1024, 128),      # 8 tiles, one per workgroup, two K-steps: prologue and tail touch
             (768, 1280, 192),      # 15 tiles on 8 workgroups: uneven shares, three steps, the X ring wraps once
             (1024, 1536, 448)]     # 24 tiles, three each, seven steps


@pytest.fixture(autouse=True)
def _persistent_variant():
    """Variant 26 sends whole-tile shapes to the persistent / in-loop-residual kernels at any size."""
    lib = L.load()
    L.check(lib.hm_gemm_set_variant(26))
    yield
    lib.hm_gemm_set_variant(-1)


def _u(name, shape, hw, seed):
    return synth.uniform(name, shape, hw, 0.0, seed=seed)


def _gemm_scaled(x, w, bias, epilogue, out_scale):
    """hm_gemm with GemmArgs.out_scale set (ops.gemm leaves it 0)."""
    M, K = x.shape
    N = w.shape[0]
    out = torch.empty(M, N, device=x.device, dtype=x.dtype)
    a = L.GemmArgs(L.ptr(x), L.ptr(w), L.ptr(out), L.ptr(bias), None, M, N, K, x.stride(0), w.stride(0), out.stride(0), 0, 0, epilogue,
                   L.HM_DTYPE_BF16 if x.dtype == torch.bfloat16 else L.HM_DTYPE_F16, None, None, None, None, 0, out_scale)
    L.check(L.load().hm_gemm(C.byref(a), L.current_stream()), "hm_gemm")
    return out


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("M,N,K", PX_SHAPES)
def test_persistent_staggered_exact(M, N, K, dt):
    """gemm_pxs_kernel on exact-integer data, eight workgroups (several tiles each), with and without bias, three launches
    each (race screen): bit-exact against torch."""
    x, w, bias, _ = ED.gemm_case(M, N, K)
    xd, wd, bd = x.to(DEV, dt), w.to(DEV, dt), bias.to(DEV)
    ref = x @ w.t()
    with L.option(L.HM_OPT_PX_GRID, 8), L.option(L.HM_OPT_GEMM_STAGGER, STAGGERED):
        for rep in range(3):
            ED.assert_exact(ops.gemm(xd, wd, bd, L.HM_EPI_STORE).float(), (ref + bias).to(dt).float(), (M, N, K, dt, "launch", rep))
        for rep in range(3):
            ED.assert_exact(ops.gemm(xd, wd, None, L.HM_EPI_STORE).float(), ref.to(dt).float(), (M, N, K, dt, "no bias", rep))


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
def test_persistent_staggered_equals_lockstep_on_random_data(dt):
    """STORE, and GELU in both epilogue forms and with out_scale != 1: the same bytes as the lockstep kernel."""
    for (M, N, K) in PX_SHAPES:
        xr = _u("sx", (M, K), 1.0, M).to(DEV, dt)
        wr = _u("sw", (N, K), 0.05, N).to(DEV, dt)
        bd = _u("sb", (N,), 0.5, K).to(DEV)
        with L.option(L.HM_OPT_PX_GRID, 8):
            got = {}
            for arm in (LOCKSTEP, STAGGERED):
                with L.option(L.HM_OPT_GEMM_STAGGER, arm):
                    outs = [ops.gemm(xr, wr, bd, L.HM_EPI_STORE)]
                    for form in (1, 2):
                        with L.option(L.HM_OPT_PX_LDS_EPILOGUE, form):
                            outs += [ops.gemm(xr, wr, bd, L.HM_EPI_STORE), ops.gemm(xr, wr, bd, L.HM_EPI_GELU),
                                     _gemm_scaled(xr, wr, bd, L.HM_EPI_GELU, 0.25)]
                    got[arm] = outs
            for i, (a, b) in enumerate(zip(got[LOCKSTEP], got[STAGGERED])):
                assert torch.equal(a, b), (M, N, K, dt, i)
            assert not torch.equal(got[STAGGERED][2], got[STAGGERED][3])            # (out_scale took effect)


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("M,N,K", ED.GEMM_INLOOP_RESIDUAL)
def test_inloop_residual_staggered_exact(M, N, K, dt):
    """gemm_x3rs_kernel on exact-integer data: exact, also in place (out aliasing resid) and without bias."""
    x, w, bias, resid = ED.gemm_case(M, N, K, resid=ED.GEMM_INLOOP_RESIDUAL_RANGE)
    xd, wd, bd, rd = x.to(DEV, dt), w.to(DEV, dt), bias.to(DEV), resid.to(DEV)
    ref = x @ w.t() + bias + resid
    with L.option(L.HM_OPT_GEMM_STAGGER, STAGGERED):
        for rep in range(3):
            ED.assert_exact(ops.gemm(xd, wd, bd, L.HM_EPI_RESID_F32, resid=rd), ref, (M, N, K, dt, "launch", rep))
        inplace = rd.clone()
        ops.gemm(xd, wd, bd, L.HM_EPI_RESID_F32, resid=inplace, out=inplace)
        ED.assert_exact(inplace, ref, (M, N, K, dt, "in place"))
        ED.assert_exact(ops.gemm(xd, wd, None, L.HM_EPI_RESID_F32, resid=rd), ref - bias, (M, N, K, dt, "no bias"))


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("M,N,K", [(256, 256, 1280), (256, 512, 5120)])
def test_inloop_residual_staggered_equals_lockstep_on_random_data(M, N, K, dt):
    """Equal bytes, not closeness: the lagging waves add R(t) behind their pending mma(t+1, 1), where the leaders add it."""
    a, wt = _u("ra", (M, K), 1.0, 1).to(DEV, dt), _u("rw", (N, K), 0.05, 2).to(DEV, dt)
    bb, rr = _u("rb", (N,), 0.5, 3).to(DEV), _u("rr", (M, N), 2.0, 4).to(DEV)
    with L.option(L.HM_OPT_GEMM_STAGGER, LOCKSTEP):
        old = ops.gemm(a, wt, bb, L.HM_EPI_RESID_F32, resid=rr)
    with L.option(L.HM_OPT_GEMM_STAGGER, STAGGERED):
        new = ops.gemm(a, wt, bb, L.HM_EPI_RESID_F32, resid=rr)
    assert torch.equal(new, old), (M, N, K, dt)


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
def test_shapes_the_staggered_kernels_do_not_take_stay_exact(dt):
    """Ragged M or N, K = 64, a residual with a row modulus, K < 1280 for the residual: option 2 falls back as option 1 does."""
    with L.option(L.HM_OPT_GEMM_STAGGER, STAGGERED):
        for (M, N, K) in [(300, 260, 128), (512, 1284, 192), (2048, 2048, 64)]:
            x, w, bias, _ = ED.gemm_case(M, N, K)
            o = ops.gemm(x.to(DEV, dt), w.to(DEV, dt), bias.to(DEV), L.HM_EPI_STORE)
            ED.assert_exact(o.float(), (x @ w.t() + bias).to(dt).float(), (M, N, K, dt, "store fall-back"))
        for (M, N, K, mod) in [(512, 256, 1280, 128), (512, 256, 1216, 0), (300, 260, 1280, 0)]:
            x, w, bias, resid = ED.gemm_case(M, N, K, resid=ED.GEMM_INLOOP_RESIDUAL_RANGE, resid_rows=mod or None)
            o = ops.gemm(x.to(DEV, dt), w.to(DEV, dt), bias.to(DEV), L.HM_EPI_RESID_F32, resid=resid.to(DEV), resid_mod=mod)
            ref = x @ w.t() + bias + (resid.repeat(M // mod, 1) if mod else resid)
            ED.assert_exact(o, ref, (M, N, K, mod, dt, "residual fall-back"))


def test_forward_of_64_crops_is_the_same_bytes():
    """One HaMeR forward at B = 64 (the shapes both staggered kernels carry): every output tensor equal under options 1 and 2."""
    L.load().hm_gemm_set_variant(-1)
    cfg = synth.HamerConfig()
    sd = synth.hamer_state_dict(cfg, seed=0, device=DEV)
    eng = HamerEngine(sd, synth.mano_params(seed=0), cfg)
    img = synth.normalize_crops(synth.crops_u8(16, seed0=0)).to(DEV).repeat(4, 1, 1, 1)
    outs = {}
    for arm in (LOCKSTEP, STAGGERED):
        with L.option(L.HM_OPT_GEMM_STAGGER, arm):
            outs[arm] = {k: v.clone() for k, v in eng.forward(img).items()}
            torch.cuda.synchronize()
    assert set(outs[LOCKSTEP]) == set(outs[STAGGERED])
    for k, v in outs[LOCKSTEP].items():
        assert torch.isfinite(v).all(), k
        assert torch.equal(v, outs[STAGGERED][k]), k


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
def test_detector_1x1_silu_layer_is_the_same_bytes(dt):
    """A 1x1 / stride 1 / SiLU layer that hm_conv2d_nhwc sends to the persistent kernel (HM_OPT_CONV_TILE = 16), input and
    output as channel slices of wider buffers."""
    lib = L.load()
    n, Ci, Co, H, W, ldx, ldy = 2, 512, 512, 48, 80, 512 + 64, 512 + 192
    x = _u("dx", (n, H, W, ldx), 1.0, 7).to(DEV, dt)
    w = _u("dw", (Co, Ci), (3.0 / Ci) ** 0.5, 8).to(DEV, dt)
    b = _u("db", (Co,), 0.3, 9).to(DEV)
    zeros = torch.zeros(64, dtype=torch.uint8, device=DEV)
    got = {}
    for arm in (LOCKSTEP, STAGGERED):
        y = torch.zeros(n, H, W, ldy, dtype=dt, device=DEV)
        a = L.ConvArgs(x.data_ptr() + 64 * 2, w.data_ptr(), y.data_ptr() + 192 * 2, b.data_ptr(), zeros.data_ptr(), n, H, W, Ci, Co, 1, 1,
                       ldx, ldy, Ci, 1, 0, L.HM_DTYPE_BF16 if dt == torch.bfloat16 else L.HM_DTYPE_F16, None, 0, None, 0)
        with L.option(L.HM_OPT_CONV_TILE, 16), L.option(L.HM_OPT_GEMM_STAGGER, arm):
            L.check(lib.hm_conv2d_nhwc(C.byref(a), L.current_stream()), "hm_conv2d_nhwc")
        torch.cuda.synchronize()
        got[arm] = y
    assert bool((got[STAGGERED][..., :192] == 0).all()) and bool((got[STAGGERED][..., 192:] != 0).any())
    assert torch.equal(got[LOCKSTEP], got[STAGGERED])
