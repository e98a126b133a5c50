"""GPU parity of the SAR hand-mesh head (csrc/sar.hip, rootnet/sar.py, EstimateRGB.run / run_frames) against the fp32 rule
of tests/sar_rule.py (which tests/test_sar_host.py pins to the reference's modules)."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sar_rule as R  # noqa: E402

from hamer_yolo_amd import ops, synth  # noqa: E402
from hamer_yolo_amd.rootnet.sar import SarHeadEngine, sar_hand  # noqa: E402
from oracle import rootnet_ref as RR  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
K = np.array([[906.96, 0, 960], [0, 906.79, 540], [0, 0, 1]])


@pytest.fixture(scope="module")
def sd():
    return synth.sar_head_state_dict(0)


@pytest.fixture(scope="module")
def eng(sd):
    return SarHeadEngine(sd, device=DEV)


def _feats(B, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.relu(torch.randn(B, 8, 8, 512, generator=g)).half()          # NHWC f16, as RootNetEngine.features


def _nchw(f):
    return f.float().permute(0, 3, 1, 2).contiguous()


def test_saigb_kernel(sd, eng):
    f = _feats(3, 1)
    g = eng.saigb(f.to(DEV)).float().cpu()                                       # [778][B][544]
    ref = R.saigb({k: v.float() for k, v in sd.items()}, _nchw(f))             # (B, 778, 515)
    np.testing.assert_allclose(g[:, :, :515].permute(1, 0, 2).numpy(), ref.numpy(), rtol=2e-3, atol=2e-3)
    assert not g[:, :, 515:].any()


def test_graph_mix_and_linear_kernels(sd, eng):
    """L . x (transposed LDS read of the [K][N] operand) and both fc epilogues, against fp32 on the same f16 operands."""
    from hamer_yolo_amd import lib as L
    B = 5
    x = (torch.randn(778, B * 544) * 0.5).half()
    y = torch.empty(778, B * 544, dtype=torch.float16, device=DEV)
    lap = eng.w["xy.lap0"]
    L.check(L.load().hm_sar_graph_mix(L.ptr(lap), 800, L.ptr(x.to(DEV)), B * 544, L.ptr(y), L.current_stream()))
    ref = lap.float().cpu()[:, :778] @ x.float()
    np.testing.assert_allclose(y.float().cpu().numpy(), ref.numpy(), rtol=2e-3, atol=2e-3)
    xs = x.reshape(778 * B, 544).to(DEV)
    for f32 in (0, 1):
        out = torch.empty(778 * B, 1024, dtype=torch.float32 if f32 else torch.float16, device=DEV)
        L.check(L.load().hm_sar_linear(L.ptr(xs), 778 * B, 544, L.ptr(eng.w["xy.w0"]), L.ptr(eng.w["xy.b0"]), L.ptr(out), 1024, f32,
                                       L.current_stream()))
        r = xs.float().cpu() @ eng.w["xy.w0"].float().cpu().T + eng.w["xy.b0"].cpu()
        if not f32:
            r = F.leaky_relu(r, 0.1)
        np.testing.assert_allclose(out.float().cpu().numpy(), r.numpy(), rtol=2e-3, atol=2e-3)


def test_softargmax_kernel(sd, eng):
    """mesh2pose + beta + softmax + coordinate sums in fp32, against the rule on the same logits."""
    B = 3
    ws = eng._workspace(B)
    g = torch.Generator().manual_seed(4)
    lx = torch.randn(778, B, 1024, generator=g) * 3
    lz = torch.randn(778, B, 1024, generator=g) * 0.1
    ws["xy"][:778].copy_(lx)
    ws["z"][:778].copy_(lz)
    got = eng.soft_argmax(B).cpu()
    ref = R.tail(sd, lx.permute(1, 0, 2), lz.permute(1, 0, 2))
    np.testing.assert_allclose(got.numpy(), ref.numpy(), rtol=0, atol=1e-5)


@pytest.mark.parametrize("B", [1, 7, 64])
def test_whole_head_against_fp32_rule(sd, eng, B):
    f = _feats(B, 10 + B)
    coords = eng.forward(f.to(DEV))
    check = sorted({0, B // 2, B - 1})                     # the rule is per hand: check a few
    ref = R.head(sd, _nchw(f[check]))
    got = coords.cpu()[check]
    err = (got - ref).abs().amax().item()
    assert err <= 2e-3, f"normalised uvd max error {err}"
    hands = [sar_hand(np.array([[0.7, 0, 500.0], [0, 0.7, 300.0]], np.float32), K, 1920, 1080, i % 2 == 1) for i in range(B)]
    root = torch.full((B,), 0.6)
    uvd, xyz = eng.postprocess(coords, hands, root)
    uvd, xyz = uvd.cpu().numpy(), xyz.cpu().numpy()
    for j, b in enumerate(check):
        out = R.post_process(ref[j].numpy(), np.float32(0.6), np.array([[0.7, 0, 500.0], [0, 0.7, 300.0]], np.float32), K, 1920, b % 2 == 1)
        assert np.abs(xyz[b, :778] - out["mesh_xyz"]).max() <= 1e-3
        assert np.abs(xyz[b, 778:] - out["pose_xyz"]).max() <= 1e-3


def test_batch_invariance(eng):
    f = _feats(64, 99).to(DEV)
    all64 = eng.forward(f).clone()
    one = eng.forward(f[13:14].contiguous())
    assert torch.equal(one[0], all64[13])


def _frame(H=720, W=1280, seed=5):
    return synth.frame_u8(H, W, seed=seed).numpy()


def test_left_hand_patch_is_the_mirrored_frames_patch():
    """generate_patch_image(do_flip=True) (rootnet/preprocessing.py:54-70): the patch of the mirrored frame at
    bb_c_x = W - bb_c_x - 1, not the crop at bb_c_x mirrored afterwards."""
    from hamer_yolo_amd.rootnet.Model_RGB import get_model
    est = get_model()
    fr = _frame()
    H, W = fr.shape[:2]
    bp = np.float32([400.5, 200.25, 300.0, 300.0])
    img, raw = est._sar_patches([torch.from_numpy(fr).to(DEV)], [(0, bp)], [True], 256)
    cx, cy = float(bp[0] + 0.5 * bp[2]), float(bp[1] + 0.5 * bp[3])
    mirrored = torch.from_numpy(np.ascontiguousarray(fr[:, ::-1])).to(DEV)
    rec = ops.crop_boxes([(W - cx - 1, cy, float(bp[2]), False)]).to(DEV)
    ref = ops.crop_batch(mirrored, rec, est.mean, est.std)
    assert torch.equal(img, ref)
    rec_hamer = ops.crop_boxes([(cx, cy, float(bp[2]), True)]).to(DEV)      # HaMeR's flip (mirror after the crop) differs
    assert not torch.equal(ops.crop_batch(torch.from_numpy(fr).to(DEV), rec_hamer, est.mean, est.std), ref)


def _rule_run(est, sd, fr, bbox, hand_type, depth_mm=None):
    """The rule's flow of run() around the head: box, patch transform, root depth (ResRootNet oracle or the depth image)
    and post-processing, on the product's own head output for that patch (the backbone and the head have their own parity
    tests)."""
    from hamer_yolo_amd.rootnet.preprocessing import process_bbox
    H, W = fr.shape[:2]
    x1, y1, x2, y2 = bbox
    bp = process_bbox([x1, y1, x2 - x1, y2 - y1], W, H, (256, 256), 1.5)
    flip = hand_type == "left"
    img, _ = est._sar_patches([torch.from_numpy(fr).to(DEV)], [(0, bp)], [flip], 256)
    feats = est.engine.features(img)
    coords = est.head.forward(feats)[0].cpu().numpy()       # the head itself: test_whole_head_against_fp32_rule
    _, bb2img = R.patch_trans(bp, flip, W)
    if depth_mm is not None:
        root = R.root_from_depth(coords, bb2img, depth_mm, W, H)
    else:
        net, rsd = synth.rootnet_state_dict(0)
        k = RR.calculate_k(bp, K[0, 0], K[1, 1])
        root = np.float32(RR.root_depth(rsd, _nchw(feats.cpu()), torch.tensor([k], dtype=torch.float32)).reshape(-1)[0].item())
    return R.post_process(coords, root, bb2img, K, W, flip), float(bb2img[0, 0]) * 256


@pytest.mark.parametrize("hand_type", ["right", "left"])
@pytest.mark.parametrize("with_depth", [False, True])
def test_run_against_rule(sd, hand_type, with_depth):
    from hamer_yolo_amd.rootnet.Model_RGB import get_model
    est = get_model()
    fr = _frame(1080, 1920, seed=7)
    bbox = [700.0, 350.0, 950.0, 620.0]
    inp = {"rgb": fr, "rgb_bbox": bbox, "hand_type": hand_type}
    depth = None
    if with_depth:
        y, x = np.mgrid[0:1080, 0:1920]
        depth = (500 + 0.05 * x + 0.08 * y).astype(np.uint16)                 # smooth: a root-pixel error of 0.1 px stays < 0.1 mm
        inp["depth"] = depth
    meta, out = est.run([inp])
    ref, px = _rule_run(est, sd, fr, bbox, hand_type, depth)
    for k in ("pose_uvd", "mesh_uvd"):
        np.testing.assert_allclose(out[k], ref[k], rtol=1e-6, atol=1e-4)
    for k in ("pose_xyz", "mesh_xyz"):
        assert out[k].dtype == np.float32 and np.abs(out[k] - ref[k]).max() <= 1e-5, k
    assert meta["crop_img_rgb"].shape == (256, 256, 3) and meta["crop_img_rgb"].dtype == np.uint8
    assert meta["pose_img_rgb"].shape == (256, 256, 3) and meta["crop_img_d"] is None and meta["cube"] == 300.0
    np.testing.assert_array_equal(meta["joint_xyz_world"], out["pose_xyz"])


def test_run_frames_equals_run():
    from hamer_yolo_amd.rootnet.Model_RGB import get_model
    est = get_model()
    frames = [_frame(1080, 1920, seed=s) for s in (11, 12)]
    dets = [[["right", [700.0, 350.0, 950.0, 620.0]], ["left", [1200.0, 400.0, 1400.0, 640.0]]], [["left", [100.0, 100.0, 300.0, 260.0]]]]
    got = est.run_frames([torch.from_numpy(f).to(DEV) for f in frames], K, dets)
    i = 0
    for fr, ds in zip(frames, dets):
        for label, box in ds:
            _, out = est.run([{"rgb": fr, "rgb_bbox": box, "hand_type": label}])
            for k in ("pose_uvd", "mesh_uvd", "pose_xyz", "mesh_xyz"):
                np.testing.assert_allclose(got[k][i].cpu().numpy(), out[k], rtol=1e-6, atol=1e-4)
            i += 1


def test_checkpoint_without_rootnet_serves_run_with_zero_root(monkeypatch):
    from hamer_yolo_amd.rootnet import Model_RGB as M
    real = M.synth.rootnet_state_dict
    monkeypatch.setattr(M.synth, "rootnet_state_dict", lambda seed=0: (real(seed)[0], None))
    est = M.get_model()
    assert est.rootnet is None
    with pytest.raises(RuntimeError):
        est.estimate_root_depth_custom(_frame(), K, [500.0, 260.0, 690.0, 470.0])
    inp = [{"rgb": _frame(), "rgb_bbox": [500.0, 260.0, 690.0, 470.0], "hand_type": "right"}]
    _, out0 = est.run(inp)
    monkeypatch.undo()
    est1 = M.get_model()
    _, out1 = est1.run(inp)
    root = est1.estimate_root_depth_custom(_frame(), est1.camera_K(), inp[0]["rgb_bbox"])
    dz = out1["mesh_xyz"][:, 2] - out0["mesh_xyz"][:, 2]                  # z = 0.3 * relative + root: root 0 without RootNet
    assert np.abs(dz - root).max() < 1e-4, (dz.min(), dz.max(), root)
