"""GPU parity of the ConvNeXt-base SAR backbone (csrc/convnext.hip, rootnet/convnext_engine.py, EstimateRGB(backbone=
'convnext')): the new kernels against fp32 torch statements of the same step, the backbone against the fp64 rule of
tests/convnext_rule.py (which tests/test_convnext_host.py pins to the reference's own module), the 1024-channel SAR head
against tests/sar_rule.py, and the estimator end to end against the fp64 chain.  Every "measured" bound is at most twice the
value measured on an MI355X, stated next to it; each test prints its figures before it asserts."""
import gc
import os
import sys
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import convnext_rule as CR  # noqa: E402
import sar_precise_chain as PC  # noqa: E402
import sar_rule as R  # noqa: E402

from hamer_yolo_amd import lib as L  # noqa: E402
from hamer_yolo_amd import synth  # noqa: E402
from hamer_yolo_amd.rootnet import convnext_arch as arch  # noqa: E402
from hamer_yolo_amd.rootnet.convnext_engine import ConvNextEngine  # noqa: E402
from hamer_yolo_amd.rootnet.sar import SarHeadEngine, sar_hand  # noqa: E402
from oracle import rootnet_ref as RR  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
K = np.array([[906.96, 0, 960], [0, 906.79, 540], [0, 0, 1]])
EPS = 1e-6
# the four stage geometries at 2 hands, the odd one of the issue (borders on every side, a partial run of 4 along x) and one
# whose channel count is no power of two (18 threads per pixel: the general reduction)
GEOMETRIES = [(2, 64, 64, 128), (2, 32, 32, 256), (2, 16, 16, 512), (2, 8, 8, 1024), (3, 12, 20, 256), (2, 10, 14, 72)]


def _cfg(**kw):
    base = dict(backbone="convnext", in_channels=1024, checkpoint="synthetic:0", device="cuda", input_img_shape=(256, 256),
                bbox_real=(0.3, 0.3), cam_para=[906.96, 906.79, 960, 540], depth_box=0.3, precise=False)
    return types.SimpleNamespace(**{**base, **kw})


@pytest.fixture(scope="module")
def net():
    return synth.convnext_state_dict(0)


@pytest.fixture(scope="module")
def root():
    return synth.convnext_rootnet_state_dict(0)


@pytest.fixture(scope="module")
def head_sd():
    return synth.sar_head_state_dict(0, in_channels=1024)


@pytest.fixture(scope="module")
def bb(net, root):
    return ConvNextEngine(net, root, device=DEV)


@pytest.fixture(scope="module")
def head(head_sd):
    return SarHeadEngine(head_sd, device=DEV, in_channels=1024)


@pytest.fixture(scope="module")
def est():
    from hamer_yolo_amd.rootnet.Model_RGB import EstimateRGB
    e = EstimateRGB(_cfg())
    assert isinstance(e.engine, ConvNextEngine) and e.head.in_channels == 1024 and e.rootnet is e.engine
    return e


def _stream(B, H, W, C, seed):
    """An fp32 NHWC stream in which a wrong tap or a wrong border shows: a ramp over x, y and the channel plus noise."""
    g = torch.Generator().manual_seed(seed)
    y, x, c = torch.arange(H).view(1, H, 1, 1), torch.arange(W).view(1, 1, W, 1), torch.arange(C).view(1, 1, 1, C)
    ramp = 0.03 * x - 0.05 * y + 0.002 * ((c * 7) % 13) * (x + 2 * y) / 8
    return (ramp + 0.1 * torch.arange(B).view(B, 1, 1, 1) + 0.5 * torch.randn(B, H, W, C, generator=g)).float().contiguous()


def _dwconv_ln(x, w, b, g, be, dtype=torch.float16):
    B, H, W, C = x.shape
    out = torch.empty(B * H * W, C, device=DEV, dtype=dtype)
    xd, wt, bd, gd, bed = (t.to(DEV) for t in (x, w.reshape(C, 49).t().contiguous(), b, g, be))      # (held until the copy back)
    L.check(L.load().hm_dwconv7_ln(L.ptr(xd), L.ptr(wt), L.ptr(bd), L.ptr(gd), L.ptr(bed), L.ptr(out), B, H, W, C,
                                   EPS, L.HM_DTYPE_F16 if dtype == torch.float16 else L.HM_DTYPE_BF16, L.current_stream()), "hm_dwconv7_ln")
    torch.cuda.synchronize()
    return out.cpu().reshape(B, H, W, C)


def _block_params(C, seed):
    w = synth.uniform("t.dw", (C, 1, 7, 7), (3.0 / 49) ** 0.5, 0.0, seed=seed)
    b = synth.uniform("t.db", (C,), 0.2, 0.0, seed=seed)
    g = synth.uniform("t.g", (C,), 0.3, 1.0, seed=seed)
    be = synth.uniform("t.b", (C,), 0.3, 0.0, seed=seed)
    return w, b, g, be


# ---------------------------------------------------------------------------------------------------------- 1. kernels
@pytest.mark.parametrize("B,H,W,C", GEOMETRIES)
def test_dwconv7_ln_kernel(B, H, W, C):
    """Depthwise 7 x 7 + LayerNorm against the fp32 torch statement of the same step; rtol = atol = 2e-3, the bound
    tests/test_gpu_sar.py uses for this project's kernels with f16 outputs."""
    x = _stream(B, H, W, C, seed=C + H)
    w, b, g, be = _block_params(C, C)
    ref = F.layer_norm(F.conv2d(x.permute(0, 3, 1, 2), w, b, padding=3, groups=C).permute(0, 2, 3, 1), (C,), g, be, EPS)
    got = _dwconv_ln(x, w, b, g, be).float()
    print(f"dwconv7_ln {B}x{H}x{W}x{C}: max err {float((got - ref).abs().max()):.3g}")
    np.testing.assert_allclose(got.numpy(), ref.numpy(), rtol=2e-3, atol=2e-3)
    if C == 256:
        got16 = _dwconv_ln(x, w, b, g, be, torch.bfloat16).float()
        np.testing.assert_allclose(got16.numpy(), ref.numpy(), rtol=1.6e-2, atol=1.6e-2)      # bf16: 8 bits of mantissa


def _patchify(x, g, be):
    B, H, W, C = x.shape
    out = torch.empty(B * (H // 2) * (W // 2), 4 * C, device=DEV, dtype=torch.float16)
    xd, gd, bed = x.to(DEV), g.to(DEV), be.to(DEV)
    L.check(L.load().hm_ln_patchify2(L.ptr(xd), L.ptr(gd), L.ptr(bed), L.ptr(out), B, H, W, C, EPS, L.HM_DTYPE_F16,
                                     L.current_stream()), "hm_ln_patchify2")
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize("B,H,W,C", GEOMETRIES)
def test_ln_patchify2_kernel(B, H, W, C):
    x = _stream(B, H, W, C, seed=3 * C + W)
    _, _, g, be = _block_params(C, C + 1)
    y = F.layer_norm(x, (C,), g, be, EPS)
    ref = y.reshape(B, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(B * (H // 2) * (W // 2), 4 * C)
    got = _patchify(x, g, be).float()
    print(f"ln_patchify2 {B}x{H}x{W}x{C}: max err {float((got - ref).abs().max()):.3g}")
    np.testing.assert_allclose(got.numpy(), ref.numpy(), rtol=2e-3, atol=2e-3)


def test_block_kernels_are_per_pixel():
    """A hand alone and the same hand at position 13 of 64 give the same bytes, in every stage geometry."""
    for H, C in ((64, 128), (32, 256), (16, 512), (8, 1024)):
        x = _stream(64, H, H, C, seed=C)
        w, b, g, be = _block_params(C, 2 * C)
        assert torch.equal(_dwconv_ln(x[13:14].contiguous(), w, b, g, be)[0], _dwconv_ln(x, w, b, g, be)[13]), (H, C)
        alone, all64 = _patchify(x[13:14].contiguous(), g, be), _patchify(x, g, be)
        n = (H // 2) ** 2
        assert torch.equal(alone, all64[13 * n:14 * n]), (H, C)


def test_stem4_im2col_moves_and_rounds():
    img = CR.patches(5, n=3)
    out = torch.empty(3 * 64 * 64, 64, device=DEV, dtype=torch.float16)
    imd = img.to(DEV)
    L.check(L.load().hm_stem4_im2col(L.ptr(imd), L.ptr(out), 3, 256, 256, L.HM_DTYPE_F16, L.current_stream()), "hm_stem4_im2col")
    got = out.cpu()
    ref = F.unfold(img, 4, stride=4).transpose(1, 2).reshape(3 * 64 * 64, 48).half()
    assert torch.equal(got[:, :48], ref)
    assert not got[:, 48:].any()


def test_saigb_ch_kernel(head_sd, head):
    g0 = torch.Generator().manual_seed(1)
    f = torch.randn(3, 8, 8, 1024, generator=g0).half()
    g = head.saigb(f.to(DEV)).float().cpu()                                     # [778][B][544]
    ref = R.saigb({k: v.float() for k, v in head_sd.items()}, f.float().permute(0, 3, 1, 2).contiguous())
    np.testing.assert_allclose(g[:, :, :515].permute(1, 0, 2).numpy(), ref.numpy(), rtol=2e-3, atol=2e-3)
    assert not g[:, :, 515:].any()
    # 512 channels: the new entry point writes the bytes of hm_sar_saigb
    sd512 = synth.sar_head_state_dict(0)
    e512 = SarHeadEngine(sd512, device=DEV)
    f512 = torch.relu(torch.randn(5, 8, 8, 512, generator=g0)).half().to(DEV)
    old = e512.saigb(f512).clone()
    new = torch.full_like(old, float("nan"))
    L.check(L.load().hm_sar_saigb_ch(L.ptr(f512), L.ptr(e512.w["saigb_w"]), L.ptr(e512.w["saigb_b"]), L.ptr(e512.w["template"]), L.ptr(new),
                                     5, 512, L.current_stream()), "hm_sar_saigb_ch")
    assert torch.equal(old.view(torch.int16), new.view(torch.int16))


# ---------------------------------------------------------------------------------------------------------- 2. backbone
# error / max |feature| (4.90) against the fp64 rule, measured on an MI355X at B = 1 / 7 / 64: max 8.76e-4 / 8.76e-4 / 9.30e-4,
# rms 1.89e-4 / 1.89e-4 / 1.88e-4; bound: twice the largest.  A CPU emulation of the same roundings on
# the reference's module (weights of this style) had put it at 8.8e-4: the maximum is one f16 ulp of the final map at 4
# (3.9e-3 = 8.0e-4 of 4.90), the rms is the accumulated part.
FEAT_VS_FP64 = 1.86e-3
# against the rule's f16 emulation (same rounding points): measured max 7.98e-4 (one ulp of the final map) at every B,
# rms 1.60e-4 / 1.61e-4 / 1.60e-4.  NOT well under the fp64 distance: a summation-order difference of 1e-7 flips a few f16 roundings in the first blocks, each
# flip is a whole ulp on one element, and by the time the differences reach a tenth of an ulp a tenth of all roundings flip -- after
# 36 blocks the two sets of rounding errors are as good as independent.  The emulation pins the SIZE of the rounding error,
# not its bits.
FEAT_VS_EMU_MAX, FEAT_VS_EMU_RMS = 1.59e-3, 3.2e-4


@pytest.mark.parametrize("B", [1, 7, 64])
def test_backbone_features_against_fp64_rule(net, bb, B):
    img = torch.cat([CR.patches(100 + i) for i in range(B)])
    feat = bb.features(img.to(DEV))
    assert feat.dtype == torch.float16 and feat.shape == (B, 8, 8, 1024) and feat.is_contiguous()
    check = sorted({0, B // 2, B - 1})                     # the rule is per hand: first, middle, last
    got = feat.cpu()[check].double()
    assert torch.isfinite(got).all()
    ref = CR.forward(net, img[check], dtype=torch.float64)
    emu = CR.forward(net, img[check], dtype=torch.float64, emu="f16")
    scale = float(ref.abs().max())
    assert scale > 1.0
    err = float((got - ref).abs().max()) / scale
    rms = float((got - ref).pow(2).mean().sqrt()) / scale
    e_max = float((got - emu).abs().max()) / scale
    e_rms = float((got - emu).pow(2).mean().sqrt()) / scale
    print(f"convnext features B={B}: max|feature| {scale:.3f}; vs fp64 max {err:.3e} rms {rms:.3e}; vs f16 emulation max {e_max:.3e} rms {e_rms:.3e}")
    assert err <= FEAT_VS_FP64, err
    assert e_max <= FEAT_VS_EMU_MAX and e_rms <= FEAT_VS_EMU_RMS, (e_max, e_rms)


def test_backbone_batch_dependence(bb):
    """Hand 13 alone against hand 13 of 64: the same bytes, measured on an MI355X.  hm_gemm picks its tile by shape (at 64 hands
    the C -> 4C GEMMs run on the persistent 256 x 256 kernel and the 4C -> C ones on the 128 x 128 tile, at 1 hand everything on
    the 128 x 128 tile; a kernel trace shows that the in-loop-residual kernel, whose 2e-5 batch dependence DESIGN section 0
    item 9 records, is not chosen for these shapes), but each of these tiles forms an output as ONE k-ordered MFMA sum from
    zero with bias and residual added behind it, and the kernels of csrc/convnext.hip are per pixel."""
    img = torch.cat([CR.patches(200 + i) for i in range(64)]).to(DEV)
    all64 = bb.features(img).clone()
    one = bb.features(img[13:14].contiguous())
    diff = float((one[0].float() - all64[13].float()).abs().max())
    print(f"convnext batch dependence, hand 13 alone vs of 64: max |difference| {diff:.3e}; bit-equal: {torch.equal(one[0], all64[13])}")
    assert torch.equal(bb.features(img), all64)             # deterministic run to run
    assert torch.equal(one[0], all64[13])


def test_root_depth_layer_on_features(bb, root):
    g = torch.Generator().manual_seed(8)
    f = torch.randn(5, 8, 8, 1024, generator=g).half()
    kv = torch.tensor([0.7, 1.0, 1.9, 2.5, 3.3])
    got = bb.depth_of(f.to(DEV), kv.to(DEV)).cpu().double()
    ref = CR.root_depth(root, f.double(), kv)
    np.testing.assert_allclose(got.numpy(), ref.numpy(), rtol=1e-5, atol=1e-6)


# ---------------------------------------------------------------------------------------------------------- 3. head
@pytest.mark.parametrize("B", [1, 7, 64])
def test_head_on_1024_channel_features(head_sd, head, B):
    """The bounds of test_whole_head_against_fp32_rule: 2e-3 normalised, 1e-3 m on mesh_xyz / pose_xyz."""
    g = torch.Generator().manual_seed(10 + B)
    f = torch.randn(B, 8, 8, 1024, generator=g).half()                        # post-LayerNorm features: unit variance, signed
    coords = head.forward(f.to(DEV))
    check = sorted({0, B // 2, B - 1})
    ref = R.head(head_sd, f[check].float().permute(0, 3, 1, 2).contiguous())
    err = (coords.cpu()[check] - ref).abs().amax().item()
    print(f"1024-channel head B={B}: normalised uvd max error {err:.3e}")
    assert err <= 2e-3, f"normalised uvd max error {err}"
    bb2img = np.array([[0.7, 0, 500.0], [0, 0.7, 300.0]], np.float32)
    hands = [sar_hand(bb2img, K, 1920, 1080, i % 2 == 1) for i in range(B)]
    uvd, xyz = head.postprocess(coords, hands, torch.full((B,), 0.6))
    xyz = xyz.cpu().numpy()
    for j, b in enumerate(check):
        out = R.post_process(ref[j].numpy(), np.float32(0.6), bb2img, K, 1920, b % 2 == 1)
        assert np.abs(xyz[b, :778] - out["mesh_xyz"]).max() <= 1e-3
        assert np.abs(xyz[b, 778:] - out["pose_xyz"]).max() <= 1e-3


# ---------------------------------------------------------------------------------------------------------- 4. end to end
def _frame(H=1080, W=1920, seed=7):
    return synth.frame_u8(H, W, seed=seed).numpy()


def _patch(est, fr, bbox, hand_type):
    from hamer_yolo_amd.rootnet.preprocessing import process_bbox
    H, W = fr.shape[:2]
    x1, y1, x2, y2 = bbox
    bp = process_bbox([x1, y1, x2 - x1, y2 - y1], W, H, (256, 256), 1.5)
    img, _ = est._sar_patches([torch.from_numpy(fr).to(DEV)], [(0, bp)], [hand_type == "left"], 256)
    return bp, img


def _head_fp64(head_sd, feat_nhwc):
    """tests/sar_precise_chain.head with the 1024-channel SAIGB (its .view(-1, 778, 512) is the output's, not the input's)."""
    return PC.head(head_sd, feat_nhwc.permute(0, 3, 1, 2).contiguous())


def _chain(net, root, head_sd, img, bp, fr, hand_type, depth_mm=None):
    """The fp64 chain on the patch the GPU cut for this hand (as tests/test_gpu_sar_precise.py does it)."""
    H, W = fr.shape[:2]
    flip = hand_type == "left"
    feat = CR.forward(net, img.cpu(), dtype=torch.float64)
    coords = _head_fp64(head_sd, feat)[0]
    _, bb2img = R.patch_trans(bp, flip, W)
    if depth_mm is not None:
        rt = R.root_from_depth(coords.float().numpy(), bb2img, depth_mm, W, H)
    else:
        rt = float(CR.root_depth(root, feat, [RR.calculate_k(bp, K[0, 0], K[1, 1])])[0])
    return R.post_process(coords.numpy(), np.float32(rt), bb2img, K, W, flip), coords, rt


def _dist(out, ref):
    d = {}
    for k in ("pose", "mesh"):
        e_xyz = np.abs(np.asarray(out[k + "_xyz"], np.float64) - ref[k + "_xyz"])
        e_uvd = np.abs(np.asarray(out[k + "_uvd"], np.float64) - ref[k + "_uvd"])
        d[k + "_xyz"], d[k + "_uv"], d[k + "_d"] = float(e_xyz.max()), float(e_uvd[:, :2].max()), float(e_uvd[:, 2].max())
    return d


# distances of run() to the fp64 chain, measured on an MI355X for a right hand / a left hand / a right hand with a depth image
# (box 403.5 px, root depth 0.75 / 0.88 / 0.58 m); bounds: twice the largest of the three
E2E_COORDS = 1.68e-3         # normalised coordinates        8.08e-4 / 8.43e-4 / 8.08e-4
E2E_UV_PER_BOX = 1.68e-3     # u, v as a share of the box    8.08e-4 / 8.43e-4 / 8.08e-4  (0.33 / 0.34 / 0.33 px)
E2E_D = 3.58e-4              # d in metres                   1.59e-4 / 1.79e-4 / 5.34e-5
E2E_XYZ_PER_M = 6.0e-4       # xyz per metre of depth        2.61e-4 / 3.01e-4 / 2.09e-4
ROOT_DEPTH_REL = 2.27e-4     # estimate_root_depth_custom    3.9e-5 / 1.14e-4 relative, two boxes


@pytest.mark.parametrize("hand_type,with_depth", [("right", False), ("left", False), ("right", True)])
def test_run_against_fp64_chain(est, net, root, head_sd, hand_type, with_depth):
    fr = _frame()
    bbox = [700.0, 350.0, 950.0, 620.0]
    inp = {"rgb": fr, "rgb_bbox": bbox, "hand_type": hand_type}
    depth = None
    if with_depth:
        y, x = np.mgrid[0:1080, 0:1920]
        depth = (500 + 0.05 * x + 0.08 * y).astype(np.uint16)
        inp["depth"] = depth
    meta, out = est.run([inp])
    bp, img = _patch(est, fr, bbox, hand_type)
    ref, coords, rt = _chain(net, root, head_sd, img, bp, fr, hand_type, depth)
    c16 = (est.head.forward(est.engine.features(img))[0].cpu().double() - coords).abs().max().item()
    box_px = float(bp[2])
    zscale = max(1.0, float(np.abs(ref["mesh_xyz"][:, 2]).max()))
    d = _dist(out, ref)
    msg = (f"convnext run {hand_type} depth={with_depth}: coords {c16:.3e}; box {box_px:.1f} px, z {zscale:.3g} m, root {rt:.4g}; "
           f"uv/box {max(d['pose_uv'], d['mesh_uv']) / box_px:.3e} ({max(d['pose_uv'], d['mesh_uv']):.3g} px); "
           f"d {max(d['pose_d'], d['mesh_d']):.3e} m; xyz/m {max(d['pose_xyz'], d['mesh_xyz']) / zscale:.3e}")
    print(msg)
    assert c16 <= E2E_COORDS, msg
    for k in ("pose", "mesh"):
        assert out[k + "_xyz"].dtype == np.float32 and d[k + "_xyz"] <= E2E_XYZ_PER_M * zscale, msg
        assert d[k + "_uv"] <= E2E_UV_PER_BOX * box_px and d[k + "_d"] <= E2E_D, msg
    assert meta["crop_img_rgb"].shape == (256, 256, 3) and meta["cube"] == 300.0
    np.testing.assert_array_equal(meta["joint_xyz_world"], out["pose_xyz"])


def test_run_frames_equals_run(est):
    frames = [_frame(seed=s) for s in (11, 12)]
    dets = [[["right", [700.0, 350.0, 950.0, 620.0]], ["left", [1200.0, 400.0, 1400.0, 640.0]]], [["left", [100.0, 100.0, 300.0, 260.0]]]]
    got = est.run_frames([torch.from_numpy(f).to(DEV) for f in frames], K, dets)
    i = 0
    for fr, ds in zip(frames, dets):
        for label, box in ds:
            _, out = est.run([{"rgb": fr, "rgb_bbox": box, "hand_type": label}])
            for k in ("pose_uvd", "mesh_uvd", "pose_xyz", "mesh_xyz"):
                np.testing.assert_array_equal(got[k][i].cpu().numpy(), out[k], err_msg=f"hand {i} {k}")
            i += 1


def test_root_depth_against_rule(est, net, root):
    """estimate_root_depth_custom against the rule's GAP + depth layer on the fp64 features of the same patch.  The depth
    is a mean over 65536 f16 features: relative error measured 3.9e-5 / 1.14e-4, bound twice the larger."""
    from hamer_yolo_amd.rootnet.preprocessing import process_bbox
    frame = synth.frame_u8(720, 1280, seed=33).numpy()
    Kc = np.array([[900.0, 0, 640], [0, 880.0, 360], [0, 0, 1]], np.float32)
    for bbox in ([500.0, 260.0, 690.0, 470.0], [100.0, 80.0, 300.0, 330.0]):
        depth = est.estimate_root_depth_custom(frame, Kc, bbox)
        x1, y1, x2, y2 = bbox
        bp = process_bbox([x1, y1, x2 - x1, y2 - y1], 1280, 720, (256, 256), 1.5)
        img = est.patch(frame, bp).cpu()
        k = RR.calculate_k(bp, float(Kc[0, 0]), float(Kc[1, 1]))
        ref = float(CR.root_depth(root, CR.forward(net, img, dtype=torch.float64), [k])[0])
        print(f"convnext root depth {bbox}: {depth:.6g} vs {ref:.6g}, relative {abs(depth - ref) / abs(ref):.3e}")
        assert abs(depth - ref) <= ROOT_DEPTH_REL * abs(ref), (depth, ref)
    batched = est.estimate_root_depths_frames([torch.from_numpy(frame).to(DEV)], Kc, [[["right", [500.0, 260.0, 690.0, 470.0]]]])
    assert batched.shape == (1,) and abs(float(batched[0]) - est.estimate_root_depth_custom(frame, Kc, [500.0, 260.0, 690.0, 470.0])) == 0.0





def test_checkpoint_without_rootnet_or_head(monkeypatch):
    from hamer_yolo_amd.rootnet import Model_RGB as M
    fr = _frame(720, 1280, seed=5)
    inp = [{"rgb": fr, "rgb_bbox": [500.0, 260.0, 690.0, 470.0], "hand_type": "right"}]
    est1 = M.EstimateRGB(_cfg())
    _, out1 = est1.run(inp)
    rt = est1.estimate_root_depth_custom(fr, est1.camera_K(), inp[0]["rgb_bbox"])
    monkeypatch.setattr(M.synth, "convnext_rootnet_state_dict", lambda seed=0: None)
    est0 = M.EstimateRGB(_cfg())
    assert est0.rootnet is None
    with pytest.raises(RuntimeError):
        est0.estimate_root_depth_custom(fr, K, [500.0, 260.0, 690.0, 470.0])
    _, out0 = est0.run(inp)
    dz = out1["mesh_xyz"][:, 2] - out0["mesh_xyz"][:, 2]                  # z = 0.3 * relative + root: root 0 without RootNet
    assert np.abs(dz - rt).max() < 1e-4, (dz.min(), dz.max(), rt)
    monkeypatch.setattr(M.synth, "sar_head_state_dict", lambda seed=0, in_channels=512: {})
    nohead = M.EstimateRGB(_cfg())
    assert nohead.head is None
    with pytest.raises(RuntimeError):
        nohead.run(inp)


def test_real_format_checkpoint_loads_without_the_classifier(tmp_path, est, net, root, head_sd):
    """The synthetic state dict with the 21841-row classifier added, saved as the reference's {'net', 'rootnet'} file: the
    product loader gives the bytes of the synthetic:0 route and the classifier (45 MB in f16, 89 MB in fp32) is not on the
    device."""
    from hamer_yolo_amd.rootnet.Model_RGB import EstimateRGB
    full = {**net, **head_sd, arch.PREFIX + "head.weight": torch.randn(arch.NUM_CLASSES, 1024) * 0.02,
            arch.PREFIX + "head.bias": torch.zeros(arch.NUM_CLASSES)}
    path = tmp_path / "SAR-convnext-root.pth"
    torch.save({"net": full, "rootnet": root}, path)
    del full
    gc.collect()
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    e = EstimateRGB(_cfg(checkpoint=str(path)))
    torch.cuda.synchronize()
    held = torch.cuda.memory_allocated() - before
    head_bytes = sum(v.numel() * v.element_size() for v in e.head.w.values())
    print(f"convnext checkpoint: engine operands {e.engine.weight_bytes() / 1e6:.1f} MB, head {head_bytes / 1e6:.1f} MB, device memory taken {held / 1e6:.1f} MB")
    assert e.engine.weight_bytes() == est.engine.weight_bytes()
    assert held <= e.engine.weight_bytes() + head_bytes + 16 * 1024 * 1024          # allocator rounding; far under the classifier
    inp = [{"rgb": _frame(720, 1280, seed=5), "rgb_bbox": [500.0, 260.0, 690.0, 470.0], "hand_type": "left"}]
    _, a = e.run(inp)
    _, b = est.run(inp)
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


# ---------------------------------------------------------------------------------------------------------- 5. d_infer
def test_d_infer_with_the_convnext_backbone(tmp_path):
    """python -m hamer_yolo_amd.d_infer --rootnet-backbone convnext on a small folder: the records of the one-hand calls
    (the shape of test_d_infer_chunked_driver_equals_one_hand_calls, its tolerances)."""
    from PIL import Image
    from hamer_yolo_amd import d_infer
    from hamer_yolo_amd.infer import hand_record
    from hamer_yolo_amd.rootnet import sar_config_stage_1 as cfgmod
    from hamer_yolo_amd.rootnet.Model_RGB import get_model

    class _Cfg:
        ckpt_path = "synthetic:0"; model_cfg = None; use_onnx = False; onnx_path = None

    frames = {"a": synth.frame_u8(480, 640, seed=8).numpy(), "b": synth.frame_u8(480, 640, seed=9).numpy()}
    dets = {"a": [["right", [100.0, 120.0, 260.0, 300.0]], ["left", [380.0, 200.0, 520.0, 330.0]]],
            "b": [["left", [30.0, 40.0, 200.0, 260.0]], ["right", [600.0, 100.0, 640.0, 101.0]]]}

    class _Det:
        def detect(self, image):
            for k, f in frames.items():
                if np.array_equal(f, image):
                    return [None], [dets[k]]
            raise AssertionError("unknown frame")
    (tmp_path / "rgb").mkdir()
    for k, f in frames.items():
        Image.fromarray(f[:, :, ::-1]).save(tmp_path / "rgb" / f"{k}.png")
    Kc = np.array([[600.0, 0, 320], [0, 610.0, 240], [0, 0, 1]], np.float32)
    old = cfgmod.rgb_opt.backbone, cfgmod.rgb_opt.in_channels
    try:
        args = d_infer._parser().parse_args(["--input", "i", "--output", "o", "--intrinsics", "k", "--rootnet-backbone", "convnext"])
        d_infer.apply_rootnet_backbone(args)
        sar = get_model()
    finally:
        cfgmod.rgb_opt.backbone, cfgmod.rgb_opt.in_channels = old
    assert isinstance(sar.engine, ConvNextEngine)
    hi = d_infer.hamer_inference(_Cfg)
    d_infer.process_batch_manopara(str(tmp_path / "rgb"), str(tmp_path / "out"), Kc, hamer=hi, detector=_Det(), sar=sar)
    assert sorted(p.name for p in (tmp_path / "out").iterdir()) == ["a.npy", "b.npy"]
    for k in "ab":
        rec = np.load(tmp_path / "out" / f"{k}.npy", allow_pickle=True).item()
        want = {"left": None, "right": None}
        for det in dets[k]:
            try:
                depth = sar.estimate_root_depth_custom(frames[k], Kc, det[1])
            except ValueError:
                continue
            out, _ = hi.estimate_from_rgb(frames[k], [det], Kc, depth_refine=depth)
            want[det[0]] = hand_record(out, det[0] == "right", 0)
        for label in ("left", "right"):
            assert (rec[label] is None) == (want[label] is None), (k, label)
            if want[label] is None:
                continue
            for key in ("betas", "theta", "cam_t"):
                np.testing.assert_allclose(rec[label][key], want[label][key], rtol=1e-4, atol=2e-4, err_msg=f"{k} {label} {key}")
