"""GPU parity of the precise (fp32) route of EstimateRGB -- the ResNet-34 backbone, ResRootNet and the SAR head in fp32
operands (csrc/conv_f32.hip hm_conv2d_f32_relu, csrc/yolo.hip hm_*_f32, csrc/sar_f32.hip) -- against the whole chain in
fp64 on the CPU (tests/sar_precise_chain.py).  Every bound is at most twice the value measured on an MI355X, stated next to
it; the default (16-bit) route's distance on the same hands is recorded to show what the route buys."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sar_precise_chain as PC  # noqa: E402
import sar_rule as R  # noqa: E402

from hamer_yolo_amd import lib as L  # noqa: E402
from hamer_yolo_amd import synth  # noqa: E402
from hamer_yolo_amd.rootnet.engine import RootNetEngine  # noqa: E402
from hamer_yolo_amd.rootnet.sar import SarHeadEngine  # noqa: E402
from oracle import rootnet_ref as RR  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
K = np.array([[906.96, 0, 960], [0, 906.79, 540], [0, 0, 1]])


@pytest.fixture(scope="module")
def sd():
    return synth.sar_head_state_dict(0)


@pytest.fixture(scope="module")
def nets():
    return synth.rootnet_state_dict(0)


@pytest.fixture(scope="module")
def bb(nets):
    return RootNetEngine(nets[0], nets[1], device=DEV, dtype=torch.float32)


@pytest.fixture(scope="module")
def eng(sd):
    return SarHeadEngine(sd, device=DEV, precise=True)


@pytest.fixture(scope="module")
def est():
    from hamer_yolo_amd.rootnet.Model_RGB import EstimateRGB
    from hamer_yolo_amd.rootnet.sar_config_stage_1 import rgb_opt
    e = EstimateRGB(rgb_opt, precise=True)
    assert e.precise and e.engine.precise and e.head.precise
    return e


@pytest.fixture(scope="module")
def est16():
    from hamer_yolo_amd.rootnet.Model_RGB import get_model
    e = get_model()
    assert not e.precise
    return e


def _nchw(f):
    return f.permute(0, 3, 1, 2).contiguous()


# ---------------------------------------------------------------------------------------------------------- 1. convolution
@pytest.mark.parametrize("k,stride,cin,cout", [(7, 2, 8, 64), (3, 1, 64, 64), (3, 2, 64, 128), (1, 2, 128, 256), (3, 1, 512, 512)])
@pytest.mark.parametrize("resid", [False, True])
def test_conv2d_f32_relu_against_fp64(k, stride, cin, cout, resid):
    """The five ResNet-34 shapes of test_gpu_rootnet.py's epilogue test, with and without an fp32 identity, against an fp64
    F.conv2d: error / (1 + sum|x * w|) measured <= 2.25e-7 on an MI355X, bound 4.5e-7."""
    N, H, W = 2, 20, 24
    x = synth.uniform("rx", (N, cin, H, W), 1.0, 0.0, seed=k)
    w = synth.uniform("rw", (cout, cin, k, k), (3.0 / (cin * k * k)) ** 0.5, 0.0, seed=cin)
    b = synth.uniform("rb", (cout,), 0.2, 0.0, seed=3)
    Ho, Wo = (H + 2 * (k // 2) - k) // stride + 1, (W + 2 * (k // 2) - k) // stride + 1
    idn = synth.uniform("ri", (N, cout, Ho, Wo), 1.0, 0.0, seed=9)
    ref = F.conv2d(x.double(), w.double(), b.double(), stride, k // 2)
    mag = F.conv2d(x.double().abs(), w.double().abs(), None, stride, k // 2)          # sum |x * w| per output
    if resid:
        ref = ref + idn.double()
    ref = F.relu(ref)
    kp = (k * k * cin + 63) // 64 * 64
    wk = torch.zeros(cout, kp)
    wk[:, :k * k * cin] = w.permute(0, 2, 3, 1).reshape(cout, -1)
    xd, wd, bd = x.permute(0, 2, 3, 1).contiguous().to(DEV), wk.to(DEV), b.to(DEV)
    idd = idn.permute(0, 2, 3, 1).contiguous().to(DEV)
    y = torch.empty(N, Ho, Wo, cout, device=DEV)
    a = L.ConvArgs(L.ptr(xd), L.ptr(wd), L.ptr(y), L.ptr(bd), None, N, H, W, cin, cout, k, stride, cin, cout, kp, 2, 0,
                   L.HM_DTYPE_F32, L.ptr(idd) if resid else None, cout if resid else 0)
    L.check(L.load().hm_conv2d_f32_relu(C.byref(a), L.current_stream()), "hm_conv2d_f32_relu")
    got = y.permute(0, 3, 1, 2).double().cpu()
    assert (got >= 0).all()
    rel = ((got - ref).abs() / (mag + 1.0)).max().item()
    print(f"conv k{k} s{stride} {cin}->{cout} resid={resid}: {rel:.3g}")
    assert rel <= 4.5e-7, f"error / (1 + sum|x*w|) = {rel:.3g}"


# ---------------------------------------------------------------------------------------------------------- 2. backbone
@pytest.mark.parametrize("B", [1, 7, 64])
def test_backbone_against_fp64(nets, bb, B):
    """Features against the fp64 backbone, hands checked: first, middle, last.  Measured <= 1.73e-6 of max|feat| (B = 64);
    bound 3.4e-6."""
    img = synth.normalize_crops(synth.crops_u8(B, seed0=5))
    feat = bb.features(img.to(DEV))
    assert feat.dtype == torch.float32 and feat.shape == (B, 8, 8, 512)
    check = sorted({0, B // 2, B - 1})
    ref = PC.backbone(nets[0], img[check])
    got = _nchw(feat.cpu()[check]).double()
    scale = ref.abs().max().item()
    assert scale > 0.1
    err = (got - ref).abs().max().item() / scale
    print(f"backbone B={B}: {err:.3g}")
    assert err <= 3.4e-6, f"backbone error / max|feat| = {err:.3g}"


def test_backbone_batch_invariance(bb):
    img = synth.normalize_crops(synth.crops_u8(64, seed0=5)).to(DEV)
    all64 = bb.features(img).clone()
    one = bb.features(img[13:14].contiguous())
    assert torch.equal(one[0], all64[13])


# ---------------------------------------------------------------------------------------------------------- 3. head
def test_head_kernels_against_fp64(sd, eng):
    """Each GEMM against the fp64 product of the same fp32 operands, error / (1 + sum|a * b|): measured 2.42e-7 (SAIGB),
    1.23e-6 (L . X: the dense Laplacian's 778-term sums), 3.16e-7 (fc); bounds at most twice that.  Rows of x past 778 hold NaN and
    must not reach the result."""
    g0 = torch.Generator().manual_seed(1)
    B = 3
    f = torch.relu(torch.randn(B, 8, 8, 512, generator=g0))
    g = eng.saigb(f.to(DEV)).cpu().double()                                        # [778][B][544]
    sdd = {k: v.double() for k, v in sd.items()}
    w, bias = sdd["head.saigb.group.0.weight"], sdd["head.saigb.group.0.bias"]
    ref = F.leaky_relu(F.conv2d(_nchw(f).double(), w, bias), 0.1).reshape(B, 778, 512)
    mag = F.conv2d(_nchw(f).double().abs(), w.abs()).reshape(B, 778, 512)
    e = ((g[:, :, :512].permute(1, 0, 2) - ref).abs() / (mag + 1)).max().item()
    print(f"saigb: {e:.3g}")
    assert e <= 4.8e-7
    assert torch.equal(g[:, :, 512:515].permute(1, 0, 2), sdd["head.saigb.template"].reshape(1, 778, 3).expand(B, 778, 3))
    assert not g[:, :, 515:].any()

    lib = L.load()
    x = torch.randn(778, B * 544, generator=g0)
    y = torch.empty(800, B * 544, device=DEV)
    xd = torch.full((800, B * 544), float("nan"), device=DEV)                     # rows past 778 must never be read
    xd[:778] = x.to(DEV)
    lap = eng.w["xy.lap0"]
    L.check(lib.hm_sar_graph_mix_f32(L.ptr(lap), 800, L.ptr(xd), B * 544, L.ptr(y), L.current_stream()))
    lapd = lap.cpu().double()[:, :778]
    ref = lapd @ x.double()
    mag = lapd.abs() @ x.double().abs()
    e = ((y[:778].cpu().double() - ref).abs() / (mag + 1)).max().item()
    print(f"graph_mix: {e:.3g}")
    assert e <= 2.4e-6
    xs = x.reshape(778 * B, 544).contiguous().to(DEV)
    for logits in (0, 1):
        out = torch.empty(778 * B, 1024, device=DEV)
        L.check(lib.hm_sar_linear_f32(L.ptr(xs), 778 * B, 544, L.ptr(eng.w["xy.w0"]), L.ptr(eng.w["xy.b0"]), L.ptr(out), 1024, logits,
                                      L.current_stream()))
        wd = eng.w["xy.w0"].cpu().double()
        r = xs.cpu().double() @ wd.T + eng.w["xy.b0"].cpu().double()
        mag = xs.cpu().double().abs() @ wd.abs().T
        if not logits:
            r = F.leaky_relu(r, 0.1)
        e = ((out.cpu().double() - r).abs() / (mag + 1)).max().item()
        print(f"linear logits={logits}: {e:.3g}")
        assert e <= 6.3e-7, logits


@pytest.mark.parametrize("B", [1, 7, 64])
def test_whole_head_against_fp64(sd, eng, B):
    """Same fp32 features, whole fp32 head against the fp64 head: normalised coordinates measured 4.5e-6 / 6.4e-6 / 4.3e-6
    at B = 1 / 7 / 64 on these random features (the backbone's sharper heatmaps reach ~1e-4 end to end, below); bound 1.2e-5."""
    g0 = torch.Generator().manual_seed(10 + B)
    f = torch.relu(torch.randn(B, 8, 8, 512, generator=g0))
    coords = eng.forward(f.to(DEV)).cpu()
    check = sorted({0, B // 2, B - 1})
    ref = PC.head(sd, _nchw(f[check]))
    err = (coords[check].double() - ref).abs().max().item()
    print(f"head B={B}: {err:.3g}")
    assert err <= 1.2e-5, f"head normalised max error {err:.3g}"


def test_head_batch_invariance(eng):
    g0 = torch.Generator().manual_seed(99)
    f = torch.relu(torch.randn(64, 8, 8, 512, generator=g0)).to(DEV)
    all64 = eng.forward(f).clone()
    one = eng.forward(f[13:14].contiguous())
    assert torch.equal(one[0], all64[13])


# ---------------------------------------------------------------------------------------------------------- 4-6. EstimateRGB
def _frame(H=1080, W=1920, seed=7):
    return synth.frame_u8(H, W, seed=seed).numpy()


def _patch(est, fr, bbox, hand_type):
    from hamer_yolo_amd.rootnet.preprocessing import process_bbox
    H, W = fr.shape[:2]
    x1, y1, x2, y2 = bbox
    bp = process_bbox([x1, y1, x2 - x1, y2 - y1], W, H, (256, 256), 1.5)
    img, _ = est._sar_patches([torch.from_numpy(fr).to(DEV)], [(0, bp)], [hand_type == "left"], 256)
    return bp, img


def _chain(sd, nets, img, bp, fr, hand_type, depth_mm=None):
    """The fp64 chain on the patch the GPU cut for this hand (the crop is shared by both routes): (post_process dict,
    coords (799, 3) double)."""
    H, W = fr.shape[:2]
    flip = hand_type == "left"
    feat = PC.backbone(nets[0], img.cpu())
    coords = PC.head(sd, feat)[0]
    if depth_mm is not None:
        root = R.root_from_depth(coords.float().numpy(), R.patch_trans(bp, flip, W)[1], depth_mm, W, H)
    else:
        root = float(PC.root_depth(nets[1], feat, [RR.calculate_k(bp, K[0, 0], K[1, 1])])[0])
    _, bb2img = R.patch_trans(bp, flip, W)
    return R.post_process(coords.numpy(), np.float32(root), bb2img, K, W, flip), coords


def _dist(out, ref):
    """max |error| per output: xyz in metres, uvd's u / v in pixels and d in metres (keys *_uv / *_d)."""
    d = {}
    for k in ("pose", "mesh"):
        e_xyz = np.abs(np.asarray(out[k + "_xyz"], np.float64) - ref[k + "_xyz"])
        e_uvd = np.abs(np.asarray(out[k + "_uvd"], np.float64) - ref[k + "_uvd"])
        d[k + "_xyz"], d[k + "_uv"], d[k + "_d"] = float(e_xyz.max()), float(e_uvd[:, :2].max()), float(e_uvd[:, 2].max())
    return d


@pytest.mark.parametrize("hand_type,with_depth", [("right", False), ("left", False), ("right", True)])
def test_run_against_fp64_chain(est, est16, sd, nets, hand_type, with_depth):
    """End to end, against the fp64 chain on the same patch.  Measured on an MI355X (right / left / right with a depth
    image), bounds at most twice the worst:
      normalised coordinates  1.07e-4 / 7.95e-5 / 1.07e-4           bound 2.1e-4   (default route: 4.0e-2 / 3.2e-2 / 4.0e-2)
      u, v in pixels / box    9.7e-5 / 5.4e-5 / 9.7e-5 (0.039 px)   bound 1.9e-4   (default: 10.5 px)
      d (metres)              3.4e-5 / 3.1e-5 / 3.2e-5              bound 6.8e-5   (default: 1.2e-2)
      xyz per metre of depth  4.3e-5 / 2.4e-5 / 3.2e-5              bound 8.5e-5   (default: 1.2e-2 m at 0.5 m)
    xyz is compared per metre of root depth: the synthetic ResRootNet puts the hand ~44 m away, where a 0.039 px error in u
    is 1.9 mm in x (1.9e-3 m precise, 0.51 m default); with the depth image (~0.5 m) it is 3.2e-5 m.  The default route
    must be at least 10x further away; it is ~370x on the coordinates and ~270x on xyz."""
    fr = _frame()
    bbox = [700.0, 350.0, 950.0, 620.0]
    inp = {"rgb": fr, "rgb_bbox": bbox, "hand_type": hand_type}
    depth = None
    if with_depth:
        y, x = np.mgrid[0:1080, 0:1920]
        depth = (500 + 0.05 * x + 0.08 * y).astype(np.uint16)
        inp["depth"] = depth
    _, out = est.run([inp])
    _, out16 = est16.run([inp])
    bp, img = _patch(est, fr, bbox, hand_type)
    ref, coords = _chain(sd, nets, img, bp, fr, hand_type, depth)
    c32 = (est.head.forward(est.engine.features(img))[0].cpu().double() - coords).abs().max().item()
    c16 = (est16.head.forward(est16.engine.features(img))[0].cpu().double() - coords).abs().max().item()
    box_px = float(bp[2])                                 # one normalised unit is the patch box: 256 patch px * bb2img scale
    zscale = max(1.0, float(np.abs(ref["mesh_xyz"][:, 2]).max()))
    d32, d16 = _dist(out, ref), _dist(out16, ref)
    msg = (f"{hand_type} depth={with_depth}: coords precise {c32:.3g} default {c16:.3g}; box {box_px} px, z {zscale:.3g} m; "
           f"precise {d32}; default {d16}")
    print(msg)
    assert c32 <= 2.1e-4, msg
    for k in ("pose", "mesh"):
        assert out[k + "_xyz"].dtype == np.float32 and d32[k + "_xyz"] <= 8.5e-5 * zscale, msg
        assert d32[k + "_uv"] <= 1.9e-4 * box_px and d32[k + "_d"] <= 6.8e-5, msg
    assert c16 >= 10 * c32, msg
    assert max(d16["mesh_xyz"], d16["pose_xyz"]) >= 10 * max(d32["mesh_xyz"], d32["pose_xyz"]), msg


def test_root_depth_against_fp64(est, nets):
    """estimate_root_depth_custom on the precise route against the fp64 root depth: relative error measured 8.2e-8 /
    1.45e-7, bound 2.8e-7 (the default route's test allows 5e-3)."""
    frame = synth.frame_u8(720, 1280, seed=33).numpy()
    Kc = np.array([[900.0, 0, 640], [0, 880.0, 360], [0, 0, 1]], np.float32)
    for bbox in ([500.0, 260.0, 690.0, 470.0], [100.0, 80.0, 300.0, 330.0]):
        depth = est.estimate_root_depth_custom(frame, Kc, bbox)
        from hamer_yolo_amd.rootnet.preprocessing import process_bbox
        x1, y1, x2, y2 = bbox
        bp = process_bbox([x1, y1, x2 - x1, y2 - y1], 1280, 720, (256, 256), 1.5)
        img = est.patch(frame, bp).cpu()
        k = RR.calculate_k(bp, float(Kc[0, 0]), float(Kc[1, 1]))
        ref = float(PC.root_depth(nets[1], PC.backbone(nets[0], img), [k])[0])
        print(f"root depth {bbox}: {abs(depth - ref) / abs(ref):.3g}")
        assert abs(depth - ref) <= 2.8e-7 * abs(ref), (depth, ref)


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


# ---------------------------------------------------------------------------------------------------------- 7. d_infer
def test_d_infer_batch_driver_precise(tmp_path, est):
    from PIL import Image
    from hamer_yolo_amd import d_infer

    class _Cfg:
        ckpt_path = "synthetic:0"; model_cfg = None; use_onnx = False; onnx_path = None

    class _Det:
        def __init__(self, dets): self.dets = dets
        def detect(self, image): return [None], [self.dets]
    frame = synth.frame_u8(480, 640, seed=8).numpy()
    (tmp_path / "rgb").mkdir()
    Image.fromarray(frame[:, :, ::-1]).save(tmp_path / "rgb" / "a.png")
    dets = [["right", [100.0, 120.0, 260.0, 300.0]], ["left", [380.0, 200.0, 520.0, 330.0]]]
    Kc = np.array([[600.0, 0, 320], [0, 610.0, 240], [0, 0, 1]], np.float32)
    hi = d_infer.hamer_inference(_Cfg)
    d_infer.process_batch_manopara(str(tmp_path / "rgb"), str(tmp_path / "out"), Kc, hamer=hi, detector=_Det(dets), sar=est)
    rec = np.load(tmp_path / "out" / "a.npy", allow_pickle=True).item()
    one = [est.estimate_root_depth_custom(frame, Kc, box) for _, box in dets]
    for (label, _), depth in zip(dets, one):
        np.testing.assert_allclose(rec[label]["cam_t"][2], depth, rtol=1e-5)
    batched = est.estimate_root_depths_frames([torch.from_numpy(frame).to(DEV)], Kc, [dets]).cpu()
    assert torch.equal(batched, torch.tensor(one, dtype=torch.float32))
