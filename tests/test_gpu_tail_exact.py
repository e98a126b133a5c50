"""The kernels that turn the networks' results into the product's outputs, on exact data, bit for bit.

hm_mano_forward (csrc/mano.hip): a dyadic MANO model, integer betas and signed-permutation rotations in un-normalised 6-D form
(tests/exact_data.py: mano_exact_case), for which every intermediate of the kernel is an fp32 value in any operation order;
rotmats, verts, joints, cam_t and kp2d equal mano_rule bit for bit at B in {1, 5, 67} and n_verts in {745, 778, 800}, with
guard rows around every output; degenerate 6-D poses (a1 = 0, a2 parallel to a1) likewise; and the smooth-random comparison of
test_gpu_kernels.py, at its own tolerances, at B = 1 and at both edges of n_verts.

hm_yolo_decode / hm_yolo_decode_batch (csrc/yolo.hip): logits of 0, +128 and -128, whose sigmoid is exactly 1/2, 1 and 0, on
grids from one cell to three workgroups and a partial one, nc 1, 3 and 80, NaN in the padding of a wide ldraw, row0 = 17,
three images with slabs longer than what is written; the whole pred buffer, sentinel rows included, equals decode_rule.
General logits meet the float64 formula within DECODE_ULP_BOUND ulp (measured on the CPU, tests/test_exact_data_host.py).

hm_gap_linear(_f32), hm_nchw3_to_nhwc8(_f32), hm_patch_im2col: integer features with HW a power of two against an int64 rule
(and one HW = 49 case against float64 with a derived bound); byte-equal layout changes; F.unfold of the window for all three
output types, with a large value in every pixel outside the window.
tests/test_exact_data_host.py shows on the CPU that each data set sees its catalogue of faults.
"""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exact_data as ED  # noqa: E402

from hamer_yolo_amd import lib as L  # noqa: E402
from hamer_yolo_amd import ops, synth  # noqa: E402

DEV = "cuda"
S_OUT = -12345.0
NAN = float("nan")
GUARD = 4
DT_CODE = {torch.bfloat16: L.HM_DTYPE_BF16, torch.float16: L.HM_DTYPE_F16, torch.float32: L.HM_DTYPE_F32}
DTYPES = [torch.bfloat16, torch.float16, torch.float32]


def _guarded(rows, width, dtype=torch.float32):
    """(GUARD + rows + GUARD, width): NaN where the kernel writes, a sentinel in the guard rows before and after."""
    buf = torch.full((rows + 2 * GUARD, width), S_OUT, dtype=dtype, device=DEV)
    buf[GUARD:GUARD + rows] = NAN
    return buf


def _guards_intact(buf, rows):
    return bool((buf[:GUARD] == S_OUT).all()) and bool((buf[GUARD + rows:] == S_OUT).all())


# ------------------------------------------------------------------------------------------------ MANO tail
MANO_OUT = {"rotmats": (16, 9), "verts": (None, 3), "joints": (21, 3), "cam_t": (1, 3), "kp2d": (21, 2)}      # rows per hand, width
MANO_MODEL_KEYS = ("v_template", "shapedirs", "posedirs", "J_regressor", "lbs_weights")


def _mano_run(mp, pose, betas, cam):
    """One hm_mano_forward launch into guarded buffers -> the five outputs on the CPU, shaped as mano_rule's."""
    B, V = pose.shape[0], mp["v_template"].shape[0]
    mpd = {k: mp[k].to(DEV).contiguous() for k in MANO_MODEL_KEYS}
    m = ops.mano_model_struct(mpd)
    pd, bd, cd = pose.to(DEV), betas.to(DEV), cam.to(DEV)
    bufs = {k: _guarded(B * (per or V), w) for k, (per, w) in MANO_OUT.items()}
    out = [L.ptr(bufs[k][GUARD:]) for k in ("rotmats", "verts", "joints", "cam_t", "kp2d")]
    L.check(L.load().hm_mano_forward(C.byref(m), L.ptr(pd), L.ptr(bd), L.ptr(cd), *out, B, ED.MANO_FOCAL, ED.MANO_IMAGE,
                                     L.current_stream()), "hm_mano_forward")
    res = {}
    for k, (per, w) in MANO_OUT.items():
        rows = B * (per or V)
        assert _guards_intact(bufs[k], rows), (k, "guard rows", B, V)
        res[k] = bufs[k][GUARD:GUARD + rows].cpu()
    res["rotmats"] = res["rotmats"].reshape(B, 16, 3, 3)
    for k in ("verts", "joints", "kp2d"):
        res[k] = res[k].reshape(B, -1, MANO_OUT[k][1])
    assert torch.equal(pd.cpu(), pose) and torch.equal(cd.cpu(), cam)
    return res


def _mano_compare(got, ref, what):
    for k in ("rotmats", "verts", "joints", "cam_t", "kp2d"):
        w = ref[k].shape[-1] if k != "rotmats" else 9
        ED.assert_exact(got[k].reshape(-1, w), ref[k].reshape(-1, w), what + (k,))


@pytest.mark.parametrize("V", ED.MANO_V)
@pytest.mark.parametrize("B", ED.MANO_B)
def test_mano_forward_exact(B, V):
    """All five outputs equal the rule bit for bit; V = 745 makes tip vertex 744 the last vertex of the last workgroup, V = 800
    fills the LDS arrays; every output sits between guard rows that must come back untouched."""
    mp, pose, betas, cam, _ = ED.mano_exact_case(B, V)
    ref = ED.mano_rule(mp, pose, betas, cam)
    _mano_compare(_mano_run(mp, pose, betas, cam), ref, (B, V))


def test_mano_forward_degenerate_poses_exact():
    """A joint with a1 = 0 (columns 0, a2 / |a2|, 0) and one with a2 = 1.5 a1 (columns a1 / |a1|, 0, 0): the rotation matrices
    are what rot6d_to_rotmat gives on the CPU, and every output equals the rule, which floors the norms at 1e-12f as the kernel."""
    from hamer_yolo_amd.hamer.utils.geometry import rot6d_to_rotmat
    B, V = ED.MANO_DEGENERATE
    mp, pose, betas, cam, _ = ED.mano_exact_case(B, V, degenerate=True)
    ref = ED.mano_rule(mp, pose, betas, cam)
    got = _mano_run(mp, pose, betas, cam)
    assert torch.equal(got["rotmats"], rot6d_to_rotmat(pose).reshape(B, 16, 3, 3))
    _mano_compare(got, ref, (B, V, "degenerate"))


@pytest.mark.parametrize("B,V", [(1, 778), (37, 745), (37, 800), (1, 745), (1, 800)])
def test_mano_forward_general_data_at_the_edges(B, V):
    """test_mano_forward_vs_oracle_and_manopth's smooth-random comparison (without its golden part), at its tolerances, at
    B = 1 and at n_verts = 745 and 800."""
    from oracle import hamer_ref as R
    mp = synth.mano_params(seed=0, n_verts=V)
    mpd = {k: v.to(DEV) for k, v in mp.items() if v.dtype == torch.float32}
    pose6d = synth.uniform("m6", (B, 96), 1.0, seed=7)
    betas = synth.uniform("mb", (B, 10), 2.0, seed=8)
    cam = synth.uniform("mc", (B, 3), 0.2, seed=9) + torch.tensor([0.9, 0.0, 0.0])
    o = ops.mano_forward(mpd, pose6d.to(DEV), betas.to(DEV), cam.to(DEV))
    Rr = R.rot6d_to_rotmat(pose6d).view(B, 16, 3, 3)
    verts, joints = R.mano_forward(mp, betas, Rr)
    cam_t = torch.stack([cam[:, 1], cam[:, 2], 2 * 5000.0 / (256.0 * cam[:, 0] + 1e-9)], -1)
    kp2d = R.perspective_projection(joints, cam_t, torch.full((B, 2), 5000.0 / 256.0))
    np.testing.assert_allclose(o["rotmats"].cpu().numpy(), Rr.numpy(), atol=2e-6)
    np.testing.assert_allclose(o["verts"].cpu().numpy(), verts.numpy(), atol=3e-6)
    np.testing.assert_allclose(o["joints"].cpu().numpy(), joints.numpy(), atol=3e-6)
    np.testing.assert_allclose(o["cam_t"].cpu().numpy(), cam_t.numpy(), rtol=1e-6)
    np.testing.assert_allclose(o["kp2d"].cpu().numpy(), kp2d.numpy(), atol=1e-5, rtol=1e-5)


# ------------------------------------------------------------------------------------------------ Detect decode
def _decode_launch(raw, nb, ny, nx, nc, ldraw, row0, rows, level, batch):
    """pred (nb, rows, no) on the CPU after one launch into a buffer full of the sentinel."""
    stride, anch = ED.decode_level(level)
    a6 = (C.c_float * 6)(*anch)
    rd = raw.to(DEV).contiguous()
    pred = torch.full((nb, rows, 5 + nc), ED.DECODE_SENTINEL, dtype=torch.float32, device=DEV)
    lib = L.load()
    if batch:
        L.check(lib.hm_yolo_decode_batch(L.ptr(rd), ldraw, L.ptr(pred), row0, ny, nx, nc, stride, a6, nb, rows, L.current_stream()),
                "hm_yolo_decode_batch")
    else:
        assert nb == 1
        L.check(lib.hm_yolo_decode(L.ptr(rd), ldraw, L.ptr(pred), row0, ny, nx, nc, stride, a6, L.current_stream()), "hm_yolo_decode")
    return pred.cpu()


@pytest.mark.parametrize("ny,nx", ED.DECODE_GRIDS)
@pytest.mark.parametrize("nb", ED.DECODE_NB)
def test_yolo_decode_exact(nb, ny, nx):
    """Every (nc, ldraw, row0, level) of ED.decode_cases() at this grid and batch: the whole pred buffer -- the rows before
    row0 and after the last row of every image too -- equals the rule; hm_yolo_decode_batch always, hm_yolo_decode where nb = 1."""
    cases = [c for c in ED.decode_cases() if c[:3] == (nb, ny, nx)]
    assert len(cases) == 12
    for _, _, _, nc, ldraw, row0, rows, level in cases:
        raw = ED.decode_exact_case(nb, ny, nx, nc, ldraw, row0, rows)
        ref = ED.decode_rule(ED.sigmoid_f32(raw), ny, nx, nc, row0, rows, level).float()
        for batch in ([True, False] if nb == 1 else [True]):
            got = _decode_launch(raw, nb, ny, nx, nc, ldraw, row0, rows, level, batch)
            ED.assert_exact(got.reshape(nb * rows, 5 + nc), ref.reshape(nb * rows, 5 + nc), (nb, ny, nx, nc, ldraw, row0, level, "batch" if batch else "single"))


@pytest.mark.parametrize("nb,ny,nx,nc,ldraw,row0,level", ED.DECODE_GENERAL)
def test_yolo_decode_general_logits_close(nb, ny, nx, nc, ldraw, row0, level):
    """Logits over +-8 with a few at +-30 and +-100 against the formula in float64 on the same fp32 logits.  The bound, in fp32
    ulps of the float64 value, is ED.DECODE_ULP_BOUND = 2 * (CPU fp32's own largest error on these inputs: 3.7 ulp for xy, 3.6
    for wh, 26.6 for the confidences) + 2 = 9.4, 9.2 and 55.2 ulp."""
    n = 3 * ny * nx
    rows = row0 + n + ED.DECODE_TAIL_ROWS
    raw = ED.decode_general_case(nb, ny, nx, nc, ldraw)
    ref = ED.decode_rule(torch.sigmoid(raw.double()), ny, nx, nc, row0, rows, level, exact=False)
    for batch in ([True, False] if nb == 1 else [True]):
        got = _decode_launch(raw, nb, ny, nx, nc, ldraw, row0, rows, level, batch)
        assert bool((got[:, :row0] == ED.DECODE_SENTINEL).all()) and bool((got[:, row0 + n:] == ED.DECODE_SENTINEL).all())
        live, want = got[:, row0:row0 + n], ref[:, row0:row0 + n]
        assert bool(live.isfinite().all())
        for k, cols in ED.DECODE_GROUPS.items():
            err = ED.ulp_error(live[..., cols], want[..., cols])
            print(f"decode general {(nb, ny, nx, nc)} {k}: {err:.2f} ulp (bound {ED.DECODE_ULP_BOUND[k]:.1f})")
            assert err <= ED.DECODE_ULP_BOUND[k], (k, err)


# ------------------------------------------------------------------------------------------------ RootNet layout kernels
def _gap_launch(feat, w, bias, kv, dtype):
    """depth (B + 1,) on the CPU: B results and the sentinel after depth[B - 1]."""
    B, HW, Cc = feat.shape
    fd, wd, kd = feat.to(dtype).to(DEV).contiguous(), w.to(DEV), kv.to(DEV)
    depth = torch.full((B + 1,), NAN, device=DEV)
    depth[B] = ED.GAP_SENTINEL
    lib = L.load()
    if dtype == torch.float32:
        L.check(lib.hm_gap_linear_f32(L.ptr(fd), HW, Cc, L.ptr(wd), bias, L.ptr(kd), L.ptr(depth), B, L.current_stream()), "hm_gap_linear_f32")
    else:
        L.check(lib.hm_gap_linear(L.ptr(fd), HW, Cc, L.ptr(wd), bias, L.ptr(kd), L.ptr(depth), B, DT_CODE[dtype], L.current_stream()), "hm_gap_linear")
    return depth.cpu()


@pytest.mark.parametrize("B", ED.GAP_B)
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16", "f32"])
def test_gap_linear_exact(dtype, B):
    """Integer features and weights, HW a power of two: the depths equal the int64 rule bit for bit at every C (waves without a
    channel, partial 256-channel sweeps, eight sweeps) and the sentinel after depth[B - 1] stays."""
    for HW in ED.GAP_HW:
        for Cc in ED.GAP_C:
            feat, w, bias, kv, ref = ED.gap_case(B, HW, Cc)
            assert torch.equal(feat.to(dtype).float(), feat)
            got = _gap_launch(feat, w, bias, kv, dtype)
            ED.assert_exact(got[:B].reshape(1, B), ref.reshape(1, B), (dtype, B, HW, Cc))
            assert float(got[B]) == ED.GAP_SENTINEL, (dtype, B, HW, Cc)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16", "f32"])
def test_gap_linear_close_at_hw_49(dtype):
    """HW = 49 (no power of two: the mean is rounded) on smooth data against float64 on the same rounded features.  The bound
    counts roundings: a channel's sum takes HW - 1 additions and one division, a thread folds C / 256 channels with one rounding
    each, the wave sum adds in 6 steps and the four partial sums in 2: every term passes through at most HW + C / 256 + 8
    roundings of relative size 2^-24, so |error| <= (HW + C / 256 + 8) * 2^-24 * sum |terms|, the terms being
    |feat| |w| / HW and |bias|, times |k_value|."""
    B, HW, Cc = ED.GAP_CLOSE
    feat = synth.uniform("gap.close.feat", (B, HW, Cc), 2.0, 0.5).to(dtype).float()
    w = synth.uniform("gap.close.w", (Cc,), 0.05)
    kv = synth.uniform("gap.close.k", (B,), 0.5, 1.5)
    bias = 0.25
    got = _gap_launch(feat, w, bias, kv, dtype)
    ref = ((feat.double().sum(1) / HW * w.double()).sum(1) + bias) * kv.double()
    terms = ((feat.double().abs().sum(1) / HW * w.double().abs()).sum(1) + abs(bias)) * kv.double().abs()
    bound = (HW + Cc / 256 + 8) * 2.0 ** -24 * terms
    err = (got[:B].double() - ref).abs()
    print(f"gap close {dtype}: err / bound {(err / bound).tolist()}")
    assert bool((err <= bound).all()), (err.tolist(), bound.tolist())
    assert float(got[B]) == ED.GAP_SENTINEL


@pytest.mark.parametrize("B,H,W", ED.NHWC8_SHAPES)
def test_nchw3_to_nhwc8_exact(B, H, W):
    """Channels 0..2 of every pixel are the permuted input byte for byte, channels 3..7 are +0, and the sentinel pixel after the
    last one is unchanged; bf16 and fp16 through hm_nchw3_to_nhwc8, fp32 through hm_nchw3_to_nhwc8_f32."""
    x = ED.nhwc8_case(B, H, W)
    xd = x.to(DEV)
    n = B * H * W
    lib = L.load()
    for dtype in DTYPES:
        y = torch.full((n + 1, 8), NAN, dtype=dtype, device=DEV)
        y[n] = S_OUT
        if dtype == torch.float32:
            L.check(lib.hm_nchw3_to_nhwc8_f32(L.ptr(xd), L.ptr(y), B, H, W, L.current_stream()), "hm_nchw3_to_nhwc8_f32")
        else:
            L.check(lib.hm_nchw3_to_nhwc8(L.ptr(xd), L.ptr(y), B, H, W, DT_CODE[dtype], L.current_stream()), "hm_nchw3_to_nhwc8")
        ref = torch.zeros(n + 1, 8, dtype=dtype)
        ref[:n, :3] = x.permute(0, 2, 3, 1).reshape(n, 3).to(dtype)
        ref[n] = S_OUT
        bits = torch.int32 if dtype == torch.float32 else torch.int16
        assert torch.equal(y.cpu().view(bits), ref.view(bits)), (dtype, B, H, W)
    assert torch.equal(xd.cpu(), x)


@pytest.mark.parametrize("B", ED.IM2COL_B)
@pytest.mark.parametrize("img_h,img_w,x0,win_w,patch,pad", ED.IM2COL_CASES)
def test_patch_im2col_exact(img_h, img_w, x0, win_w, patch, pad, B):
    """F.unfold of the window for bf16, fp16 and fp32 patches (fp32: the pixels bit for bit); every pixel outside the window
    holds 32768, so a read past the window shows where the padding must be zero; guard rows around the output stay."""
    img = ED.im2col_case(B, img_h, img_w, x0, win_w, patch, pad)
    gh, gw = (img_h + 2 * pad - patch) // patch + 1, (win_w + 2 * pad - patch) // patch + 1
    rows, kper = B * gh * gw, 3 * patch * patch
    imd = img.to(DEV)
    for dtype in DTYPES:
        out = _guarded(rows, kper, dtype)
        L.check(L.load().hm_patch_im2col(L.ptr(imd), L.ptr(out[GUARD:]), B, img_h, img_w, x0, win_w, patch, pad, DT_CODE[dtype],
                                         L.current_stream()), "hm_patch_im2col")
        assert _guards_intact(out, rows), (dtype, "guard rows")
        ED.assert_exact(out[GUARD:GUARD + rows].float(), ED.im2col_rule(img, x0, win_w, patch, pad, dtype), (dtype, img_h, img_w, x0, win_w, patch, pad, B))
    assert torch.equal(ops.patch_im2col(imd, x0, win_w, patch, pad, torch.float16).cpu().float(), ED.im2col_rule(img, x0, win_w, patch, pad, torch.float16))
