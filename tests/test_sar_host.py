"""Host checks of the SAR hand-mesh head (EstimateRGB.run, rootnet/Model_RGB.py:76-177, :428-570): the fp32 rule of
tests/sar_rule.py against the fixture written from the reference's own modules (tools/gen_golden_sar.py), the head's weight
mapping, the post-processing arithmetic and the calibration of the synthetic weights.  No GPU."""
import os
import sys
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sar_rule as R  # noqa: E402

from hamer_yolo_amd import synth  # noqa: E402
from hamer_yolo_amd.rootnet import sar as S  # noqa: E402
from hamer_yolo_amd.rootnet.Model_RGB import EstimateRGB, draw_2d_skeleton  # noqa: E402
from hamer_yolo_amd.rootnet.preprocessing import patch_transforms  # noqa: E402

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sar_head.npz"))
K = np.array([[906.96, 0, 960], [0, 906.79, 540], [0, 0, 1]])


def _depth_map_mm(H, W):
    y, x = np.mgrid[0:H, 0:W]
    return (400 + (37 * x + 101 * y) % 997).astype(np.uint16)


def test_rule_matches_reference_head():
    sd = synth.sar_head_state_dict(0)
    got = R.head(sd, torch.from_numpy(GOLD["feats"]).float())
    np.testing.assert_allclose(got.numpy(), GOLD["coords"], rtol=0, atol=1e-6)


def test_synthetic_heatmaps_are_peaked():
    """Calibration: a near-uniform softmax puts every coordinate at the centre and parity would prove nothing."""
    assert GOLD["max_prob"].mean() >= 0.05
    cells = (GOLD["coords"][:, :, :2] + 1) * 16
    assert np.ptp(cells[:, :, 0]) >= 8 and np.ptp(cells[:, :, 1]) >= 8


def test_head_key_mapping_and_laplacian():
    sd = synth.sar_head_state_dict(3)
    w = S.host_weights(sd)
    for br in ("xy", "z"):
        for layer, name in (("0", "lap0"), ("3", "lap1")):
            adj = sd[f"head.gbbmr.reg_{br}.{layer}.adj"]
            lap = torch.sum(adj, 1, keepdim=True) + 1e-5
            lap = 1 / lap * adj
            assert w[f"{br}.{name}"].shape == (778, 800)
            assert torch.equal(w[f"{br}.{name}"][:, :778], lap) and not w[f"{br}.{name}"][:, 778:].any()
        w0 = w[f"{br}.w0"]
        assert w0.shape == (1024, 544) and torch.equal(w0[:, :515], sd[f"head.gbbmr.reg_{br}.0.fc.weight"])
        assert not w0[:, 515:].any()
        assert torch.equal(w[f"{br}.w1"], sd[f"head.gbbmr.reg_{br}.3.fc.weight"])
    assert torch.equal(w["xy.m2p_w"], sd["head.gbbmr.mesh2pose_hm.weight"]) and torch.equal(w["z.m2p_b"], sd["head.gbbmr.mesh2pose_dm.bias"])
    assert torch.equal(w["saigb_w"], sd["head.saigb.group.0.weight"].reshape(6224, 512))
    assert torch.equal(w["beta"], sd["head.gbbmr.soft_heatmap.beta.weight"].reshape(799))
    assert torch.equal(w["wx"].reshape(32, 32)[5], torch.arange(32.0)) and torch.equal(w["wy"].reshape(32, 32)[:, 7], torch.arange(32.0))
    sd.pop("head.gbbmr.reg_z.3.adj")
    try:
        S.host_weights(sd)
        raise AssertionError("a missing head key must raise")
    except KeyError as e:
        assert "reg_z.3.adj" in str(e)


def test_rule_post_processing_matches_reference():
    for i, flip in enumerate((False, True)):
        out = R.post_process(GOLD["coords"][i], GOLD["roots"][i], GOLD["bb2img"][i], GOLD["K"], 1920, flip)
        uvd = np.concatenate([out["mesh_uvd"], out["pose_uvd"]])
        xyz = np.concatenate([out["mesh_xyz"], out["pose_xyz"]])
        np.testing.assert_allclose(uvd, GOLD["post"][i][:, :3], rtol=0, atol=1e-6 * 2000)
        np.testing.assert_allclose(xyz, GOLD["post"][i][:, 3:], rtol=0, atol=1e-6)
    np.testing.assert_array_equal(R.uvd2xyz(np.array([[1000.0, 400.0, 0.6], [-20.0, 1500.0, 1.25]], np.float32), GOLD["K"]),
                                  GOLD["uvd2xyz_out"])


def test_rule_depth_image_root_matches_reference():
    d = _depth_map_mm(1080, 1920)
    for i in range(2):
        r = R.root_from_depth(GOLD["coords"][i], GOLD["bb2img"][i], d, 1920, 1080)
        assert abs(r - GOLD["depth_roots"][i]) <= 1e-6


def test_post_processing_known_answers():
    """(uv + 0.5) * 256 (not the commented-out (uv + 1) * 128), z * 0.3 + root, the flip x -> W - x - 1, uvd2xyz."""
    c = np.zeros((799, 3), np.float32)
    c[0] = [0.0, 0.0, 0.0]
    c[1] = [-0.5, 0.25, 1.0]
    ident = np.array([[1, 0, 0], [0, 1, 0]], np.float32)
    out = R.post_process(c, 0.5, ident, K, 1000, False)
    np.testing.assert_array_equal(out["mesh_uvd"][0], [128.0, 128.0, 0.5])
    np.testing.assert_array_equal(out["mesh_uvd"][1], [0.0, 192.0, np.float32(np.float32(0.3) + np.float32(0.5))])
    flipped = R.post_process(c, 0.5, ident, K, 1000, True)
    np.testing.assert_array_equal(flipped["mesh_uvd"][0], [1000 - 128 - 1, 128.0, 0.5])
    np.testing.assert_allclose(out["mesh_xyz"][0], [(128 - 960) * 0.5 / 906.96, (128 - 540) * 0.5 / 906.79, 0.5], rtol=1e-6)


def test_product_host_post_processing_and_transforms_match_rule():
    est = object.__new__(EstimateRGB)
    est.cfg = types.SimpleNamespace(depth_box=0.3, input_img_shape=(256, 256), cam_para=[906.96, 906.79, 960, 540])
    for i, flip in enumerate((False, True)):
        meta = {"crop_img": [np.zeros((256, 256, 3), np.uint8)], "root_depth": np.float32([GOLD["roots"][i]]),
                "bb2img_trans": [GOLD["bb2img"][i]], "img2bb_trans": [GOLD["bb2img"][i]], "K": [GOLD["K"]]}
        res, meta_out = est.post_processing({"coords": GOLD["coords"][i:i + 1].copy()}, meta, 1920, flip)
        np.testing.assert_allclose(np.concatenate([res["mesh_uvd"][0], res["pose_uvd"][0]]), GOLD["post"][i][:, :3], rtol=0, atol=2e-3)
        np.testing.assert_allclose(np.concatenate([res["mesh_xyz"][0], res["pose_xyz"][0]]), GOLD["post"][i][:, 3:], rtol=0, atol=1e-6)
        assert meta_out["cube"] == 300.0 and meta_out["M"].shape == (1, 3, 3) and meta_out["pose_img_rgb"].shape == (256, 256, 3)
    for box, flip in (([100.25, 50.5, 180.0, 180.0], False), ([1500.0, 700.0, 333.5, 333.5], True)):
        box = np.float32(box)
        a, b = patch_transforms(box, flip, 1920)
        ra, rb = R.patch_trans(box, flip, 1920)
        np.testing.assert_array_equal(a, ra)
        np.testing.assert_array_equal(b, rb)
        # the two maps are inverse to each other, and the patch centre lands on the (mirrored) box centre
        cx = float(box[0] + 0.5 * box[2])
        np.testing.assert_allclose(b @ np.array([128.0, 128.0, 1.0]), [1920 - cx - 1 if flip else cx, box[1] + 0.5 * box[3]], rtol=1e-6)
    uvd = torch.tensor([[[0.0, 0.0, 0.1]]])
    inv = torch.tensor([[2.0, 0.0, 10.0], [0.0, 2.0, 20.0]])
    np.testing.assert_array_equal(est.convert2origin_pixel(uvd, inv).numpy(), [[[266.0, 276.0]]])


def test_skeleton_rule():
    img = np.zeros((64, 64, 3), np.uint8)
    uv = np.stack([np.linspace(10, 50, 21), np.full(21, 30.7)], 1)
    out = draw_2d_skeleton(img, uv)
    assert not img.any()                                   # drawn on a copy
    np.testing.assert_array_equal(out[28, 10], [255, 0, 0])                 # joint 0's disc (its centre row carries later bones)
    np.testing.assert_array_equal(out[30, int(uv[20, 0])], [255, 0, 255])   # joint 20 colour
    assert out[30 + 2, 10].any() and not out[30 + 3, 10].any()              # radius 2 disc


def test_convnext_backbone_is_refused_clearly():
    cfg = types.SimpleNamespace(backbone="convnext", checkpoint="synthetic:0", device="cuda")
    try:
        EstimateRGB(cfg)
        raise AssertionError("backbone='convnext' must raise")
    except NotImplementedError as e:
        assert "convnext" in str(e)
