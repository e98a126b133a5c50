"""CPU: the skeleton drawing rule (tests/skeleton_rule.py, the numpy statement of hm_skeleton_overlay) pinned to the host rule
it generalises, the argument checks of its C ABI (they run before any device work), the drivers' flags, the OpenPose
thickness arithmetic and the palettes."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import skeleton_rule as SR
from hamer_yolo_amd import build, infer, d_infer, lib as L, render
from hamer_yolo_amd.rootnet import Model_RGB

HM_ERR_ARG = -1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ the rule
def _random_pose(rng, H, W):
    kp = rng.uniform([-10, -10], [W + 10, H + 10], (21, 2)).astype(np.float32)
    kp[rng.integers(1, 21)] = kp[0]                                       # a bone of length 0 (or a pair of equal discs)
    return kp


@pytest.mark.parametrize("seed", range(12))
def test_rule_at_sar_radii_is_the_host_rule(seed):
    """Style 'sar' (radius 0 / 2, interleaved, COLOR_HAND_JOINTS) is Model_RGB.draw_2d_skeleton, byte for byte, joints outside
    the image and coincident joints included."""
    rng = np.random.default_rng(seed)
    H, W = 48, 64
    img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    kp = _random_pose(rng, H, W)
    order, lr, jr = render.SKELETON_STYLES["sar"]
    assert (order, lr, jr) == (L.HM_SKEL_INTERLEAVED, 0, 2)
    got = SR.draw(img[None], kp[None], [(0, lr, jr, 0.1)], render.skeleton_palette("sar"), order)[0]
    want = Model_RGB.draw_2d_skeleton(img, kp)
    assert (want != img).any() and np.array_equal(got, want)


def test_rule_orders_and_absent_joints():
    img = np.zeros((40, 40, 3), np.uint8)
    pal = np.arange(63, dtype=np.uint8).reshape(21, 3) + 1
    kp = np.full((21, 3), 1.0, np.float32)
    kp[:, :2] = [[5 + (j % 5) * 7, 5 + (j // 5) * 7] for j in range(21)]
    inter = SR.draw(img[None], kp[None], [(0, 1, 3, 0.1)], pal, SR.INTERLEAVED)[0]
    first = SR.draw(img[None], kp[None], [(0, 1, 3, 0.1)], pal, SR.BONES_FIRST)[0]
    # bones first: every disc is whole; interleaved: bone 2 (1 -> 2) runs over disc 1
    for j in range(21):
        x, y = int(kp[j, 0]), int(kp[j, 1])
        assert tuple(first[y, x]) == tuple(pal[j])
    assert tuple(inter[5, 12]) == tuple(pal[2]) and not np.array_equal(inter, first)
    # a joint at the threshold, a NaN joint and one far outside: no disc, no bone that touches them
    kp2 = kp.copy()
    kp2[2, 2] = 0.1                                                        # conf > threshold is false
    kp2[6, 0] = np.nan
    kp2[10, 1] = 1e9
    cut = SR.draw(img[None], kp2[None], [(0, 1, 3, 0.1)], pal, SR.BONES_FIRST)[0]
    colours = {tuple(c) for c in cut.reshape(-1, 3)}
    for j in (2, 6, 10):
        assert tuple(pal[j]) not in colours
    for j in (3, 7, 11):                                                   # their children keep the disc and lose the bone
        assert tuple(cut[int(kp[j, 1]), int(kp[j, 0])]) == tuple(pal[j])
        assert (cut == pal[j]).all(-1).sum() == len(SR._offsets(3))
    assert tuple(pal[1]) in colours and tuple(pal[20]) in colours


# ------------------------------------------------------------------ the C ABI
def test_exports_are_in_header_binding_and_build_list():
    header = open(os.path.join(ROOT, "include", "hamer_hip.h")).read()
    for name in ("hm_skeleton_overlay_workspace_bytes", "hm_skeleton_overlay"):
        assert re.search(r"\b%s\(" % name, header) and name in L.EXPORTS
    assert "skeleton.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "skeleton.hip"))
    assert re.search(r"enum \{ HM_SKEL_INTERLEAVED = 0, HM_SKEL_BONES_FIRST = 1 \}", header)
    assert (L.HM_SKEL_INTERLEAVED, L.HM_SKEL_BONES_FIRST) == (0, 1)
    m = re.search(r"typedef struct hm_skeleton \{(.*?)\} hm_skeleton;", header, re.S)
    fields = re.findall(r"\b(image|line_radius|joint_radius|threshold)\b(?=[,;])", m.group(1))
    assert fields == [f for f, _ in L.Skeleton._fields_] and C.sizeof(L.Skeleton) == 16


def test_version_is_unchanged():
    header = open(os.path.join(ROOT, "include", "hamer_hip.h")).read()
    assert re.search(r"#define HM_VERSION 402\b", header) and L.HM_VERSION == 402
    assert L.load().hm_version() == 402


def _call(lib, N=1, H=32, W=32, stride=2, hands=((0, 1, 3),), images=0x1000, kp=0x2000, table=True, palette=True, order=0,
          out=0x1000, ws=0x3000, ws_bytes=None):
    n = len(hands)
    tab = (L.Skeleton * max(n, 1))()
    for i, (im, lr, jr) in enumerate(hands):
        tab[i].image, tab[i].line_radius, tab[i].joint_radius, tab[i].threshold = im, lr, jr, 0.1
    pal = (C.c_uint8 * 63)()
    if ws_bytes is None:
        ws_bytes = lib.hm_skeleton_overlay_workspace_bytes(N, H, W, n) if N > 0 and H > 0 and W > 0 else 1 << 20
    return lib.hm_skeleton_overlay(images, N, H, W, kp, stride, tab if table else None, n, pal if palette else None, order, out,
                                   ws, ws_bytes, None)


BAD = {
    "N 0": dict(N=0), "N negative": dict(N=-1), "H 0": dict(H=0), "W 0": dict(W=0), "H too large": dict(H=16385),
    "W too large": dict(W=16385), "stride 1": dict(stride=1), "stride 4": dict(stride=4),
    "line radius -1": dict(hands=((0, -1, 3),)), "line radius 33": dict(hands=((0, 33, 3),)),
    "joint radius -1": dict(hands=((0, 1, -1),)), "joint radius 33": dict(hands=((0, 1, 33),)),
    "image -1": dict(hands=((-1, 1, 3),)), "image N": dict(N=2, hands=((0, 1, 3), (2, 1, 3))),
    "null images": dict(images=None), "null out": dict(out=None), "null kp": dict(kp=None), "null table": dict(table=False),
    "null palette": dict(palette=False), "null workspace": dict(ws=None), "small workspace": dict(ws_bytes=255),
    "unknown order": dict(order=2),
}


@pytest.mark.parametrize("case", sorted(BAD))
def test_bad_arguments_return_err_arg_before_any_device_work(case):
    """The pointers are made up: a call that got past the checks would have to touch them."""
    lib = L.load()
    assert _call(lib, **BAD[case]) == HM_ERR_ARG
    assert b"hm_skeleton_overlay" in lib.hm_last_error_string()


def test_small_workspace_is_one_byte_short():
    lib = L.load()
    need = lib.hm_skeleton_overlay_workspace_bytes(2, 100, 131, 3)
    assert need > 0 and _call(lib, N=2, H=100, W=131, hands=((0, 1, 3),) * 3, ws_bytes=need - 1) == HM_ERR_ARG
    assert lib.hm_skeleton_overlay_workspace_bytes(0, 100, 131, 3) == 0


def test_python_argument_checks_need_no_gpu():
    with pytest.raises(ValueError):
        render.skeleton_frames(np.zeros((1, 8, 8, 3), np.uint8), np.zeros((1, 21, 2), np.float32), [0])      # not a GPU tensor
    with pytest.raises(ValueError):
        render.skeleton_palette("nope")
    with pytest.raises(ValueError):
        render._per_hand(33, None, 2, "line_radius")
    with pytest.raises(ValueError):
        render._per_hand(None, None, 2, "line_radius")
    assert render._per_hand(None, 1, 3, "line_radius") == [1, 1, 1] and render._per_hand([0, 2], 1, 2, "joint_radius") == [0, 2]
    sig = inspect.signature(render.skeleton_frames)
    assert list(sig.parameters) == ["images_dev", "keypoints", "image_index", "style", "line_radius", "joint_radius", "threshold",
                                    "out", "inplace"]
    assert sig.parameters["style"].default == "hamer" and sig.parameters["threshold"].default == 0.1
    p = inspect.signature(render.render_folder).parameters
    assert (p["keypoints"].default, p["keypoint_style"].default, p["line_radius"].default, p["joint_radius"].default) == \
        (None, "hamer", None, None)
    assert inspect.signature(Model_RGB.EstimateRGB.run_frames).parameters["draw"].default is False
    with pytest.raises(ValueError):
        render.render_folder("a", "b", "c", None, keypoints="under")


# ------------------------------------------------------------------ drivers
@pytest.mark.parametrize("mod,base", [(infer, ["--input", "a", "--output", "b"]),
                                      (d_infer, ["--input", "a", "--output", "b", "--intrinsics", "k.txt"])])
def test_parser_flags_and_defaults(mod, base, capsys):
    ap = mod._parser()
    a = ap.parse_args(base)
    assert (a.render, a.render_style, a.render_keypoints, a.keypoint_style, a.keypoint_line_radius, a.keypoint_joint_radius) == \
        (None, "flat", None, "hamer", None, None)
    assert infer.render_keypoint_args(ap, a) == {"keypoints": None, "keypoint_style": "hamer", "line_radius": None,
                                                 "joint_radius": None}
    a = ap.parse_args(base + ["--render", "out", "--render-keypoints", "over", "--keypoint-style", "openpose",
                              "--keypoint-line-radius", "2", "--keypoint-joint-radius", "5"])
    assert infer.render_keypoint_args(ap, a) == {"keypoints": "over", "keypoint_style": "openpose", "line_radius": 2,
                                                 "joint_radius": 5}
    assert ap.parse_args(base + ["--render", "out", "--render-keypoints", "only"]).render_keypoints == "only"
    with pytest.raises(SystemExit):                                        # needs --render
        infer.render_keypoint_args(ap, ap.parse_args(base + ["--render-keypoints", "over"]))
    with pytest.raises(SystemExit):
        ap.parse_args(base + ["--render", "out", "--render-keypoints", "under"])
    with pytest.raises(SystemExit):
        infer.render_keypoint_args(ap, ap.parse_args(base + ["--render", "out", "--keypoint-line-radius", "33"]))
    capsys.readouterr()


# ------------------------------------------------------------------ OpenPose thickness
def test_openpose_radii_known_answers():
    kp = np.ones((21, 3), np.float32)
    kp[:, 0] = np.linspace(800, 900, 21)
    kp[:, 1] = np.linspace(400, 520, 21)
    # 1920 wide, "height" 3 (the reference's img.shape[2]): ratio = min(1, max(100 / 1920, 120 / 3)) = 1,
    # thickness ratio = max(round(sqrt(5760) / 50), 2) = 2 -> ring radius 1, ring thickness 2, line thickness round(1.5) = 2
    assert render.openpose_radii(1080, 1920, kp) == (1, 2)
    assert render.openpose_radii(7, 1920, kp) == (1, 2)                    # H does not enter
    assert render.openpose_radii(1080, 1920, kp[:, :2]) == (1, 2)          # no confidence column: every joint counts
    # a very wide frame: sqrt(3 * 30000) / 50 = 6 -> R 3, T 6, line round(4.5) = 4 (half to even)
    assert render.openpose_radii(1080, 30000, kp) == (2, 6)
    # a hand flatter than 0.15 px and narrower than 5 % of the width: ratio <= 0.05, thickness ratio 2, cv2 thickness -1 -> 1
    flat = kp.copy()
    flat[:, 0] = np.linspace(800, 850, 21)
    flat[:, 1] = 400 + np.linspace(0, 0.09, 21)
    assert render.openpose_radii(1080, 1920, flat) == (1, 1)
    # nothing above the rectangle's threshold, or a rectangle of area 0: the reference draws nothing
    low = kp.copy(); low[:, 2] = 0.1
    assert render.openpose_radii(1080, 1920, low) is None
    line = kp.copy(); line[:, 1] = 400
    assert render.openpose_radii(1080, 1920, line) is None


# ------------------------------------------------------------------ palettes (the reference's literals)
VIS_TOOL = [(255, 0, 0), (0, 102, 0), (0, 153, 0), (0, 204, 0), (0, 255, 0), (0, 0, 153), (0, 0, 255), (51, 51, 255),
            (102, 102, 255), (0, 102, 102), (0, 153, 153), (0, 204, 204), (0, 255, 255), (102, 102, 0), (153, 153, 0),
            (204, 204, 0), (255, 255, 0), (102, 0, 102), (153, 0, 153), (204, 0, 204), (255, 0, 255)]
HAMER = VIS_TOOL[:5] + [(0, 0, 102), (0, 0, 153), (0, 0, 204), (0, 0, 255)] + VIS_TOOL[9:]
OPENPOSE = [(100, 100, 100), (100, 0, 0), (150, 0, 0), (200, 0, 0), (255, 0, 0), (100, 100, 0), (150, 150, 0), (200, 200, 0),
            (255, 255, 0), (0, 100, 50), (0, 150, 75), (0, 200, 100), (0, 255, 125), (0, 50, 100), (0, 75, 150), (0, 100, 200),
            (0, 125, 255), (100, 0, 100), (150, 0, 150), (200, 0, 200), (255, 0, 255)]


@pytest.mark.parametrize("style,want,order,radii", [("sar", VIS_TOOL, 0, (0, 2)), ("hamer", HAMER, 0, (1, 3)),
                                                    ("openpose", OPENPOSE, 1, (None, None))])
def test_palettes_orders_and_default_radii(style, want, order, radii):
    pal = render.skeleton_palette(style)
    assert pal.dtype == np.uint8 and pal.shape == (21, 3) and [tuple(int(v) for v in c) for c in pal] == want
    assert render.SKELETON_STYLES[style] == (order,) + radii


def test_compat_modules_resolve_like_pose_utils():
    import importlib
    import sys
    from hamer_yolo_amd import compat
    compat.install()
    try:
        a = importlib.import_module("hamer.utils.draw_2d_skeleton")
        b = importlib.import_module("hamer.utils.render_openpose")
        import hamer_yolo_amd.hamer.utils.draw_2d_skeleton as A
        import hamer_yolo_amd.hamer.utils.render_openpose as B
        assert a is A and b is B
        assert callable(a.draw_2d_skeleton) and len(a.color_hand_joints) == 21
        for name in ("render_hand_keypoints", "render_openpose", "get_keypoints_rectangle"):
            assert callable(getattr(b, name))
        kp = np.array([[0, 0, 1.0], [4, 2, 1.0], [9, 9, 0.05]])
        assert b.get_keypoints_rectangle(kp, 0.1) == (4.0, 2.0, 8.0) and b.get_keypoints_rectangle(kp, 2.0) == (0, 0, 0)
    finally:
        compat.uninstall()
        for k in [k for k in sys.modules if k == "hamer" or k.startswith("hamer.")]:
            sys.modules.pop(k, None)
