"""GPU: the skeleton kernels (hm_skeleton_overlay, csrc/skeleton.hip) against the sequential numpy statement of the drawing
rule (tests/skeleton_rule.py), equal bytes everywhere, and what stands on them: render.skeleton_frames, the compat drawing
modules, render_folder(keypoints=...) and EstimateRGB.run_frames(draw=True), end to end with synthetic weights."""
import numpy as np
import pytest
import torch

import render_rule as RR
import skeleton_rule as SR
from hamer_yolo_amd import render, synth
from hamer_yolo_amd.rootnet import Model_RGB

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _images(N, H, W, seed):
    return np.stack([synth.frame_u8(H, W, seed=seed + n).numpy() for n in range(N)])


def _gpu(images, kp, index, **kw):
    return render.skeleton_frames(torch.from_numpy(images).to(DEV), torch.from_numpy(np.asarray(kp, np.float32)).to(DEV), index,
                                  **kw).cpu().numpy()


def _rule(images, kp, index, style="hamer", line_radius=None, joint_radius=None, threshold=0.1):
    order, lr, jr = render.SKELETON_STYLES[style]
    n = len(index)
    lr = np.broadcast_to(lr if line_radius is None else line_radius, (n,))
    jr = np.broadcast_to(jr if joint_radius is None else joint_radius, (n,))
    hands = [(index[i], int(lr[i]), int(jr[i]), threshold) for i in range(n)]
    return SR.draw(images, np.asarray(kp, np.float32), hands, render.skeleton_palette(style), order)


def _random_hand(rng, x0, y0, x1, y1):
    return rng.uniform([x0, y0], [x1, y1], (21, 2)).astype(np.float32)


# ------------------------------------------------------------------ case 1
def test_one_hand_sar_equals_rule_and_host_rule():
    images = _images(1, 256, 256, seed=1)
    kp = _random_hand(np.random.default_rng(1), 20, 20, 236, 236)[None]
    got = _gpu(images, kp, [0], style="sar")
    assert np.array_equal(got, _rule(images, kp, [0], style="sar"))
    assert np.array_equal(got[0], Model_RGB.draw_2d_skeleton(images[0], kp[0])) and (got != images).any()


# ------------------------------------------------------------------ case 2: the shared small scene
def _special_hand(rng, ox, oy, frac):
    """Joints 0..12 by design, at integer offset (ox, oy) (its parity decides which way the .5 ties round) plus a fraction that
    truncation removes; 13..20 random."""
    p = np.array([[0, 0], [4, 2], [0, 0], [2, 4], [0, 0],          # bones 1..4: (0,0)->(4,2), (4,2)->(0,0) and the y-major twins
                  [40, 0], [40, 40], [70, 70], [70, 70],             # bone 5 horizontal, 6 vertical, 7 at 45 degrees, 8 of length 0
                  [-35, 10], [20, -42], [120, 20], [50, 90]],        # left of, above, right of and below a 96 x 131 image
                 np.float32) + np.float32([ox, oy])
    p = np.concatenate([p, rng.uniform([0, 0], [130, 95], (8, 2)).astype(np.float32)])
    return (p + np.sign(p) * np.float32(frac)).astype(np.float32)   # away from zero, so the truncated point is p


def _scene():
    rng = np.random.default_rng(2)
    H, W = 96, 131
    images = _images(2, H, W, seed=20)
    kp = np.stack([_special_hand(rng, 20, 30, 0.25), _special_hand(rng, 21, 31, 0.75), _random_hand(rng, -10, -10, 140, 105),
                   _random_hand(rng, 0, 0, 131, 96), _random_hand(rng, 30, 20, 100, 80), _random_hand(rng, -20.5, -20.5, 60, 60)])
    return images, kp, [0, 0, 0, 1, 1, 1]


SCENE = _scene()


def test_special_hand_is_what_it_says():
    pts, present = SR.points(SCENE[1][0])
    assert present.all() and pts[:5].tolist() == [[20, 30], [24, 32], [20, 30], [22, 34], [20, 30]]
    assert pts[7].tolist() == pts[8].tolist() == [90, 100] and pts[9].tolist() == [-15, 40] and pts[10].tolist() == [40, -12]
    pts1, _ = SR.points(SCENE[1][1])
    assert pts1[:2].tolist() == [[21, 31], [25, 33]]
    # the ties: (0,0)->(4,2) has y = 0.5 and 1.5 at i = 1, 3; half-to-even sends them to 30, 32 at offset 30 and 32, 32 at 31
    t = np.linspace(0.0, 1.0, 5)
    assert np.rint(30 + t * 2).tolist() == [30, 30, 31, 32, 32] and np.rint(31 + t * 2).tolist() == [31, 32, 32, 32, 33]


@pytest.mark.parametrize("style", ["sar", "hamer"])
def test_small_scene_equals_rule(style):
    images, kp, index = SCENE
    got = _gpu(images, kp, index, style=style)
    want = _rule(images, kp, index, style=style)
    assert (want != images).any(-1).sum() > 500 and np.array_equal(got, want)


# ------------------------------------------------------------------ case 3
def test_full_hd_four_hands_and_a_long_bone():
    rng = np.random.default_rng(3)
    H, W = 1080, 1920
    images = _images(1, H, W, seed=30)
    kp = np.stack([_random_hand(rng, 600, 300, 900, 640), _random_hand(rng, 800, 350, 1100, 700),
                   _random_hand(rng, 1500, 800, 1990, 1100), _random_hand(rng, 100, 100, 400, 400)])
    kp[3, 0], kp[3, 1] = [60.5, 40.5], [1850.5, 1020.5]                  # bone 1: m = 1790
    got = _gpu(images, kp, [0] * 4)
    want = _rule(images, kp, [0] * 4)
    assert np.array_equal(got, want) and (want != images).any()


# ------------------------------------------------------------------ case 4
def test_radii_and_orders():
    images, kp, index = SCENE
    dev_images, dev_kp = torch.from_numpy(images).to(DEV), torch.from_numpy(kp).to(DEV)
    for style in ("hamer", "openpose"):                                   # interleaved, bones first
        for lr in (1, 2, 3):
            for jr in (3, 4, 5, 6):
                got = render.skeleton_frames(dev_images, dev_kp, index, style=style, line_radius=lr, joint_radius=jr).cpu().numpy()
                assert np.array_equal(got, _rule(images, kp, index, style, lr, jr)), (style, lr, jr)
    # a radius per hand, 0 and the largest among them
    lr, jr = [0, 3, 1, 32, 2, 0], [0, 6, 32, 1, 4, 2]
    got = _gpu(images, kp, index, style="openpose", line_radius=lr, joint_radius=jr)
    assert np.array_equal(got, _rule(images, kp, index, "openpose", lr, jr))


def test_orders_differ_on_this_scene():
    images, kp, index = SCENE
    pal = render.skeleton_palette("hamer")
    hands = [(i, 2, 5, 0.1) for i in index]
    assert not np.array_equal(SR.draw(images, kp, hands, pal, SR.INTERLEAVED), SR.draw(images, kp, hands, pal, SR.BONES_FIRST))


# ------------------------------------------------------------------ case 5
def test_confidences_at_below_and_above_the_threshold():
    images, kp, index = SCENE
    rng = np.random.default_rng(5)
    conf = rng.choice(np.float32([0.3, 0.29999998, 0.30000004, 0.0, 1.0, -1.0, np.nan]), (len(kp), 21, 1))
    conf[0, :4, 0] = [0.3, 0.29999998, 0.30000004, 0.3]                   # at, below, above, at
    kp3 = np.concatenate([kp, conf], -1).astype(np.float32)
    want = {style: _rule(images, kp3, index, style, 1, 3, threshold=0.3) for style in ("hamer", "openpose")}
    for style in want:
        got = _gpu(images, kp3, index, style=style, threshold=0.3, line_radius=1, joint_radius=3)
        assert np.array_equal(got, want[style])
    all_on = _rule(images, np.concatenate([kp, np.ones_like(conf)], -1), index, "hamer", 1, 3, threshold=0.3)
    assert not np.array_equal(want["hamer"], all_on) and np.array_equal(all_on, _rule(images, kp, index, "hamer", 1, 3))


# ------------------------------------------------------------------ case 6
def test_non_finite_and_out_of_range_joints_are_left_out():
    images, kp, index = SCENE
    bad = kp.copy()
    bad[0, 1, 0] = np.nan
    bad[0, 6, 1] = np.inf
    bad[1, 5] = [-np.inf, 10]
    bad[2, 0, 0] = 1e9                                                      # the wrist: five bones go with it
    bad[3, 9, 1] = -1e9
    bad[4, 2] = [32768.0, 40.0]                                            # |u| >= 32768: absent
    bad[5, 3] = [32767.5, -32767.5]                                        # present, far outside: bones 3 and 4 are 32000 px long
    got = _gpu(images, bad, index)
    want = _rule(images, bad, index)
    assert np.array_equal(got, want)
    pts, present = SR.points(bad[5])
    assert present[3] and pts[3].tolist() == [32767, -32767] and not SR.points(bad[4])[1][2]
    # everything else is drawn: the hands whose joints are all present and in range draw what they drew
    assert (want != images).any() and not np.array_equal(want, _rule(images, kp, index))


# ------------------------------------------------------------------ cases 7, 8
def test_deterministic_and_in_place_equals_out_of_place():
    images, kp, index = SCENE
    dev_images, dev_kp = torch.from_numpy(images).to(DEV), torch.from_numpy(kp).to(DEV)
    a = render.skeleton_frames(dev_images, dev_kp, index, line_radius=2, joint_radius=4)
    b = render.skeleton_frames(dev_images, dev_kp, index, line_radius=2, joint_radius=4)
    assert torch.equal(a, b) and torch.equal(dev_images.cpu(), torch.from_numpy(images))      # the input is not written
    out = torch.empty_like(dev_images)
    assert render.skeleton_frames(dev_images, dev_kp, index, line_radius=2, joint_radius=4, out=out) is out and torch.equal(out, a)
    work = dev_images.clone()
    assert render.skeleton_frames(work, dev_kp, index, line_radius=2, joint_radius=4, inplace=True) is work
    assert torch.equal(work, a)


# ------------------------------------------------------------------ case 9
def test_shuffling_hands_that_do_not_overlap():
    rng = np.random.default_rng(9)
    H, W = 100, 150
    images = _images(2, H, W, seed=90)
    boxes = [(5, 5, 65, 40), (85, 5, 145, 40), (5, 60, 65, 95), (85, 60, 145, 95)]                 # 20 px apart, radii <= 3
    kp = np.stack([_random_hand(rng, *boxes[i % 4]) for i in range(8)])
    index = [i // 4 for i in range(8)]
    base = _gpu(images, kp, index)
    assert np.array_equal(base, _rule(images, kp, index))
    for seed in (0, 1):
        perm = np.random.default_rng(seed).permutation(8)
        assert np.array_equal(_gpu(images, kp[perm], [index[p] for p in perm]), base)


# ------------------------------------------------------------------ case 10
def test_image_without_hands_and_no_hands_at_all():
    images = _images(3, 50, 70, seed=100)
    kp = _random_hand(np.random.default_rng(10), 0, 0, 70, 50)[None].repeat(2, 0)
    got = _gpu(images, kp, [2, 0])
    assert np.array_equal(got[1], images[1]) and np.array_equal(got, _rule(images, kp, [2, 0]))
    dev = torch.from_numpy(images).to(DEV)
    none = render.skeleton_frames(dev, torch.zeros(0, 21, 2, device=DEV), [])
    assert none is not dev and torch.equal(none, dev)
    assert render.skeleton_frames(dev, np.zeros((0, 21, 2), np.float32), [], inplace=True) is dev and torch.equal(dev.cpu(), torch.from_numpy(images))
    # a hand wholly outside the image, and one with every joint absent
    off = np.stack([kp[0] + np.float32(500), np.full((21, 2), np.nan, np.float32)])
    assert np.array_equal(_gpu(images, off, [0, 1]), images)


# ------------------------------------------------------------------ the other paths of the launch code
def test_more_hands_than_one_gather_and_than_one_setup_launch():
    """70 hands in one image (the raster kernel gathers 64 at a time) and 150 in the call (setup takes 128 per launch), table
    order interleaving the images."""
    rng = np.random.default_rng(11)
    H, W = 40, 50
    images = _images(3, H, W, seed=110)
    index = [0] * 70 + [1] * 45 + [2] * 35
    index = [index[i] for i in rng.permutation(150)]
    kp = np.stack([_random_hand(rng, -5, -5, 55, 45) for _ in range(150)])
    kp[:, 5:] = np.nan                                                      # four bones each: later hands leave earlier ones visible
    got = _gpu(images, kp, index, line_radius=0, joint_radius=1)
    assert np.array_equal(got, _rule(images, kp, index, line_radius=0, joint_radius=1))


def test_pixel_offsets_past_2_31():
    """The largest image, 16384 x 16384, with a hand in its last corner, against the rule; and the last image of a batch of
    three, which starts 1.6e9 bytes in and ends past 2^31: the hand drawn there equals the hand drawn into the batch of one,
    and nothing else is written."""
    H = W = 16384
    kp = _random_hand(np.random.default_rng(12), 16000, 16100, 16390, 16390)[None]
    one = render.skeleton_frames(torch.zeros(1, H, W, 3, dtype=torch.uint8, device=DEV), kp, [0], inplace=True)
    order, lr, jr = render.SKELETON_STYLES["hamer"]
    want = SR.draw_hand(np.zeros((H, W, 3), np.uint8), kp[0], render.skeleton_palette("hamer"), lr, jr, order)
    assert np.array_equal(one[0, 15900:, 15900:].cpu().numpy(), want[15900:, 15900:]) and want[15900:, 15900:].any()
    assert not bool(one[0, :15900].any()) and not bool(one[0, 15900:, :15900].any())
    del want
    big = torch.zeros(3, H, W, 3, dtype=torch.uint8, device=DEV)
    render.skeleton_frames(big, kp, [2], inplace=True)
    assert torch.equal(big[2], one[0]) and not bool(big[:2].any())


# ------------------------------------------------------------------ compat modules
def test_compat_modules_draw_by_the_rule():
    from hamer_yolo_amd.hamer.utils.draw_2d_skeleton import draw_2d_skeleton
    from hamer_yolo_amd.hamer.utils.render_openpose import render_hand_keypoints, render_openpose
    images, kp, _ = SCENE
    got = draw_2d_skeleton(images[0], kp[2])
    assert np.array_equal(got, _rule(images[:1], kp[2:3], [0], "hamer")[0])
    kp3 = np.concatenate([kp[4], np.ones((21, 1), np.float32)], -1)
    kp3[7, 2] = 0.05
    lr, jr = render.openpose_radii(96, 131, kp3)
    want = _rule(images[:1], kp3[None], [0], "openpose", lr, jr)[0]
    assert np.array_equal(render_openpose(images[0], kp3), want) and (want != images[0]).any()
    as_float = render_hand_keypoints(images[0].astype(np.float32), kp3)
    assert as_float.dtype == np.float32 and np.array_equal(as_float, want.astype(np.float32))
    nothing = kp3.copy(); nothing[:, 2] = 0.0
    assert np.array_equal(render_openpose(images[0], nothing), images[0])


# ------------------------------------------------------------------ case 11: the folder path, synthetic weights
class _Cfg:
    ckpt_path = "synthetic:0"
    model_cfg = None
    use_onnx = False
    onnx_path = None


class _FixedDetector:
    def __init__(self, dets):
        self.dets = dets

    def detect(self, image):
        return [None], [self.dets]


def _decode(path):
    from PIL import Image
    with Image.open(path) as im:
        return np.asarray(im.convert("RGB"))[:, :, ::-1]


def _project(points, K):
    """Section 8's projection in numpy fp64, left to right, rounded once to fp32; z <= 0 -> NaN."""
    p = np.asarray(points, np.float64)
    x, y, z0 = p[..., 0], p[..., 1], p[..., 2]
    z = np.where(z0 == 0.0, 1e-5, z0)
    w = K[2, 0] * x + K[2, 1] * y + K[2, 2] * z
    u = (K[0, 0] * x + K[0, 1] * y + K[0, 2] * z) / w
    v = (K[1, 0] * x + K[1, 1] * y + K[1, 2] * z) / w
    uv = np.stack([u, v], -1)
    return np.where((z0 > 0.0)[..., None], uv, np.nan).astype(np.float32)


def test_render_folder_keypoints_only_and_over(tmp_path):
    from PIL import Image
    from hamer_yolo_amd.infer import hamer_inference, process_batch_manopara
    hi = hamer_inference(_Cfg)
    img_dir, npy_dir = tmp_path / "rgb", tmp_path / "npy"
    img_dir.mkdir()
    H, W = 240, 320
    frames = {}
    for i in range(3):
        fr = synth.frame_u8(H, W, seed=50 + i).numpy()
        frames[f"f{i}"] = fr
        Image.fromarray(fr[:, :, ::-1]).save(img_dir / f"f{i}.bmp")
    dets = [["right", [60.0, 50.0, 150.0, 160.0]], ["left", [170.0, 80.0, 260.0, 190.0]]]
    process_batch_manopara(str(img_dir), str(npy_dir), None, hamer=hi, detector=_FixedDetector(dets))
    K = render.default_camera(H, W, hi.cfg)
    faces = np.asarray(hi.mano.faces, np.int32)
    runs = {"only": dict(keypoints="only"), "over": dict(keypoints="over"),
            "sar": dict(keypoints="over", keypoint_style="sar", line_radius=2, joint_radius=4)}
    for name, kw in runs.items():
        assert render.render_folder(str(img_dir), str(npy_dir), str(tmp_path / name), hi, ext=".bmp", frames_per_pass=2, **kw) == 3
    drawn = 0
    for stem, fr in frames.items():
        data = np.load(npy_dir / f"{stem}.npy", allow_pickle=True).item()
        hands = [data[t] for t in ("right", "left") if data[t] is not None]
        joints, verts = render.camera_joints_vertices(hi, hands)
        assert torch.equal(verts, render.camera_vertices(hi, hands))
        kp = _project(joints.cpu().numpy(), K)
        assert np.array_equal(render.project_points(joints, K).cpu().numpy(), kp, equal_nan=True)
        cam = verts.cpu().numpy().astype(np.float64)
        meshes = [{"frame": 0, "vertices": cam[j], "faces": faces, "face_id0": j * len(faces)} for j in range(len(hands))]
        mesh = RR.overlay(fr[None], K, meshes)
        index = [0] * len(hands)
        want = {"only": _rule(fr[None], kp, index)[0], "over": _rule(mesh, kp, index)[0],
                "sar": _rule(mesh, kp, index, "sar", 2, 4)[0]}
        for name in runs:
            assert np.array_equal(_decode(tmp_path / name / f"{stem}.bmp"), want[name]), (stem, name)
        drawn += int((want["only"] != fr).any())
    assert drawn == 3


# ------------------------------------------------------------------ case 12: the SAR patches
def test_run_frames_draw_equals_run():
    from hamer_yolo_amd.rootnet.sar_config_stage_1 import rgb_opt
    est = Model_RGB.EstimateRGB(rgb_opt, precise=True)                      # the fp32 route: a hand's numbers do not depend on the batch
    frames = [synth.frame_u8(480, 640, seed=s).numpy() for s in (61, 62)]
    dets = [[["right", [200.0, 150.0, 330.0, 290.0]], ["left", [380.0, 180.0, 500.0, 320.0]]], [["left", [60.0, 60.0, 200.0, 190.0]]]]
    K = est.camera_K()
    got = est.run_frames([torch.from_numpy(f).to(DEV) for f in frames], K, dets, draw=True)
    P = int(rgb_opt.input_img_shape[0])
    assert got["crop_img_rgb"].shape == got["pose_img_rgb"].shape == (3, P, P, 3) and got["pose_img_rgb"].dtype == torch.uint8
    plain = est.run_frames([torch.from_numpy(f).to(DEV) for f in frames], K, dets)
    assert set(plain) == {"pose_uvd", "mesh_uvd", "pose_xyz", "mesh_xyz"}
    assert all(torch.equal(plain[k], got[k]) for k in plain)
    i = 0
    for fr, ds in zip(frames, dets):
        for label, box in ds:
            meta, _ = est.run([{"rgb": fr, "rgb_bbox": box, "hand_type": label}])
            assert np.array_equal(got["crop_img_rgb"][i].cpu().numpy(), meta["crop_img_rgb"]), (i, label)
            assert np.array_equal(got["pose_img_rgb"][i].cpu().numpy(), meta["pose_img_rgb"]), (i, label)
            assert (meta["pose_img_rgb"] != meta["crop_img_rgb"]).any()
            i += 1
    empty = est.run_frames([torch.from_numpy(frames[0]).to(DEV)], K, [[]], draw=True)
    assert empty["pose_img_rgb"].shape == (0, P, P, 3)
