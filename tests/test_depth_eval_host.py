"""Host checks of the depth residuals (hm_depth_residuals, hamer.utils.depth_eval, hamer_yolo_amd.evaluate_depth): the numpy rule
of tests/depth_eval_rule.py against a brute-force sorted-residual median and against its own pixel-by-pixel form; the refine
loop on renders of tests/zrender_rule.py; the host summary; and the surface -- exports, header, build list, argument checks,
the drivers' parsers, the depth-map loaders.  No GPU."""
import ctypes as C
import inspect
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import depth_eval_rule as DR  # noqa: E402
import zrender_rule as ZR  # noqa: E402

from hamer_yolo_amd import build as B  # noqa: E402
from hamer_yolo_amd import lib as L  # noqa: E402
from hamer_yolo_amd.hamer.utils import depth_eval as DE  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def random_maps(seed, N=2, H=19, W=23, n_meshes=4, spread=0.05):
    rng = np.random.default_rng(seed)
    pid = rng.integers(-1, n_meshes + 1, (N, H, W)).astype(np.int32)                  # n_meshes itself: an id outside the table
    pid[rng.random((N, H, W)) < 0.3] = -1
    depth = np.where(pid >= 0, rng.uniform(0.3, 0.9, (N, H, W)), 0.0).astype(np.float32)
    sensor = np.rint((depth + rng.normal(0, spread, (N, H, W))) * 1000.0).clip(0, 65535).astype(np.uint16)
    sensor[rng.random((N, H, W)) < 0.1] = 0
    mask = rng.choice(np.array([0, 3, 5], np.uint8), (N, H, W))
    return depth, pid, sensor, mask


# ------------------------------------------------------------------ the rule
@pytest.mark.parametrize("bins,bin_m,spread", [(4096, 0.0005, 0.05), (64, 0.0005, 0.05), (2, 0.001, 0.0005), (4096, 0.0005, 3.0)])
def test_rule_against_brute_force(bins, bin_m, spread):
    for seed in (1, 2, 3):
        depth, pid, sensor, _ = random_maps(seed, spread=spread)
        mq = np.array([0, 1, 0, -1])
        hist, counts = DR.residuals(depth, pid, sensor, mq, 2, bin_m=bin_m, bins=bins)
        loop = DR.residuals_loop(depth, pid, sensor, mq, 2, bin_m=bin_m, bins=bins)
        assert np.array_equal(hist, loop[0]) and np.array_equal(counts, loop[1])
        st = DR.stats(hist, counts, bin_m)
        for q in range(2):
            sel = np.isin(pid, np.nonzero(mq == q)[0])
            assert counts[q, 0] == sel.sum() and counts[q, 1] == 0 and counts[q, 2] == (sel & (sensor == 0)).sum()
            sel &= sensor != 0
            r = sensor[sel].astype(np.float64) * 0.001 - depth[sel].astype(np.float64)
            k = np.sort(np.floor(r / bin_m).astype(np.int64) + bins // 2)
            assert counts[q, 3] == (k < 0).sum() and counts[q, 4] == (k >= bins).sum() and counts[q, 5] == ((k >= 0) & (k < bins)).sum()
            assert counts[q, 6] == counts[q, 7] == 0 and hist[q].sum() == counts[q, 5]
            mid = k[(len(k) + 1) // 2 - 1]                                             # the lower median of the sorted bins
            if 0 <= mid < bins:
                assert st[q, 0] == (mid - bins // 2 + 0.5) * bin_m
            else:
                assert np.isnan(st[q, 0])
            inside = k[(k >= 0) & (k < bins)]
            if len(inside):
                c = (inside - bins // 2 + 0.5) * bin_m
                assert np.allclose(st[q, 1:], [c.mean(), np.abs(c).mean(), np.sqrt((c * c).mean())], rtol=1e-12, atol=0)
            else:
                assert np.isnan(st[q, 1:]).all()


def test_rule_mask_labels_and_gate():
    depth, pid, sensor, mask = random_maps(7)
    mq = np.array([0, 1, 2, 3])
    for labels in ([-2, -1, 3, 5], [-2, -2, -2, -2], [3, 3, 3, 3]):
        hist, counts = DR.residuals(depth, pid, sensor, mq, 4, mask=mask, labels=labels, raw_range=(400, 800))
        loop = DR.residuals_loop(depth, pid, sensor, mq, 4, mask=mask, labels=labels, raw_range=(400, 800))
        assert np.array_equal(hist, loop[0]) and np.array_equal(counts, loop[1])
        for q, lab in enumerate(labels):
            sel = pid == q
            off = np.zeros_like(sel) if lab == -2 else sel & ~(mask != 0 if lab == -1 else mask == lab)
            assert counts[q, 1] == off.sum()
            assert counts[q, 2] == (sel & ~off & ((sensor < 400) | (sensor > 800))).sum()
            assert counts[q, 0] == counts[q, 1:6].sum()
    plain = DR.residuals(depth, pid, sensor, mq, 4)
    assert all(np.array_equal(a, b) for a, b in zip(plain, DR.residuals(depth, pid, sensor, mq, 4, mask=mask, labels=None)))
    empty = DR.stats(np.zeros((1, 8), np.int64), np.zeros((1, 8), np.int64), 0.0005)
    assert np.isnan(empty).all()
    # the rank falls in `below`: no median, the means stay defined
    h, c = np.zeros((1, 4), np.int64), np.zeros((1, 8), np.int64)
    h[0, 1], c[0, 3], c[0, 5] = 2, 5, 2
    st = DR.stats(h, c, 0.5)
    assert np.isnan(st[0, 0]) and st[0, 1] == -0.25 and st[0, 2] == 0.25 and st[0, 3] == 0.25


def test_contraction_would_show():
    depth, pid, sensor = DR.contraction_maps(4, 3, 37, 53, 5)
    r = sensor.reshape(-1).astype(np.float64) * 0.001 - depth.reshape(-1).astype(np.float64)
    plain = np.floor(r / 0.0005).astype(np.int64) + 2048
    fused = DR.fused_bins(depth, sensor)
    cov = pid.reshape(-1) >= 0
    print("pixels whose bin a fused multiply-subtract changes:", int((plain != fused)[cov].sum()), "of", int(cov.sum()))
    assert (plain != fused)[cov].sum() > 100 and (np.abs(plain - fused) <= 1).all()
    hist, counts = DR.residuals(depth, pid, sensor, [0, 1, 0, -1, 2], 3)
    assert np.array_equal(hist[1], np.bincount(plain[pid.reshape(-1) == 1], minlength=4096)) and counts[:, 5].sum() == hist.sum()


def test_summary_from_hist():
    depth, pid, sensor, _ = random_maps(9, spread=0.008)
    mq = np.array([0, 1, 2, -1])
    hist, counts = DR.residuals(depth, pid, sensor, mq, 4, bins=64)                     # query 3 has no mesh
    got, want = DE.summary_from_hist(hist, counts, 0.0005), DR.summary(hist, counts, 0.0005)
    assert sorted(got) == sorted(want) == ["covered", "inliers", "mean_abs", "measured", "median", "occluded", "valid"]
    for k in want:
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k], equal_nan=True), k
    assert np.isnan(got["median"][3]) and np.isnan(got["measured"][3]) and got["valid"][3] == 0
    assert got["inliers"].shape == (4, 3) and (got["inliers"][:3, 0] <= got["inliers"][:3, 2]).all()
    assert (got["occluded"][:3] > 0).all() and (got["measured"][:3] < 1).all()        # 64 bins of 0.5 mm: most residuals fall outside
    two = DE.summary_from_hist(torch.from_numpy(hist.astype(np.int32)), torch.from_numpy(counts), 0.0005, thresholds_m=(0.002,))
    assert two["inliers"].shape == (4, 1) and np.array_equal(two["median"], got["median"], equal_nan=True)
    none = DE.summary_from_hist(np.zeros((0, 64)), np.zeros((0, 8)), 0.0005)
    assert none["median"].shape == (0,) and none["inliers"].shape == (0, 3)
    ds = DE.dataset_summary(hist, counts, 0.0005)
    ok = np.isfinite(want["median"])
    assert ds["hands"] == 4 and ds["scored"] == ok.sum() and list(ds["inliers"]) == ["5mm", "10mm", "20mm"]
    if ok.any():
        assert ds["median_abs_mm"] == np.median(np.abs(want["median"][ok])) * 1000.0
    valid = want["valid"].sum()
    assert abs(ds["occluded"] - counts[:, 3].sum() / valid) <= 1e-15 and abs(ds["measured"] - valid / counts[:, 0].sum()) <= 1e-15
    cs = (np.arange(64) - 32 + 0.5) * 0.0005
    assert abs(ds["inliers"]["5mm"] - hist[:, np.abs(cs) <= 0.005].sum() / valid) <= 1e-15
    nothing = DE.dataset_summary(np.zeros((0, 64)), np.zeros((0, 8)), 0.0005)
    assert nothing["hands"] == 0 and np.isnan(nothing["median_abs_mm"]) and np.isnan(nothing["measured"])


# ------------------------------------------------------------------ the refine loop on the rule's renders
SCENE = dict(H=240, W=320, K=np.array([[600.0, 0, 160.0], [0, 600.0, 120.0], [0, 0, 1.0]]), centre=np.array([0.03, -0.02, 0.5]),
             factors=(1.16, 0.85, 1.4), wall=1.5, unit=0.001)


def scene_renderer(faces, H=SCENE["H"], W=SCENE["W"], K=SCENE["K"]):
    """render(placed (B, V, 3)) -> (depth, mesh_id) with hand j alone in view j, by the z-buffer rule."""
    def render(placed):
        meshes = [{"frame": j, "vertices": placed[j], "faces": faces, "face_id0": j * len(faces)} for j in range(len(placed))]
        r = ZR.render(len(placed), H, W, K, meshes)
        return r["depth"], r["mesh_id"]
    return render


def test_refine_loop_on_the_ellipsoid():
    v, f = DR.ellipsoid()
    assert len(v) == 2 + 23 * 48 and len(f) == 2 * 48 + 2 * 22 * 48 and f.min() == 0 and f.max() == len(v) - 1
    render = scene_renderer(f)
    fac = np.asarray(SCENE["factors"])
    verts = np.repeat(v[None].astype(np.float32), 3, 0)
    truth = (SCENE["centre"][None, :] * fac[:, None]).astype(np.float32)
    depth, mid = render(verts + truth[:, None, :])
    assert all((mid[j] == j).sum() > 2000 for j in range(3))
    sensor = DR.sensor_from_depth(depth, SCENE["unit"], SCENE["wall"])
    start = np.repeat(SCENE["centre"][None].astype(np.float32), 3, 0)
    cam_t, median, valid, updated, trail = DR.refine(render, verts, start, sensor, SCENE["unit"])
    e0 = np.abs(start[:, 2].astype(np.float64) - truth[:, 2])
    e1 = np.abs(trail[0][:, 2].astype(np.float64) - truth[:, 2])
    e2 = np.abs(cam_t[:, 2].astype(np.float64) - truth[:, 2])
    print("tz errors in mm: start", e0 * 1e3, "one step", e1 * 1e3, "two steps", e2 * 1e3)
    assert updated.all() and (valid >= 200).all() and cam_t.dtype == np.float32
    assert (e1 < e0).all() and (e2 <= 0.002).all()
    # the origin moved along its own ray: its pixel stayed where it was
    assert np.allclose(cam_t[:, :2] / cam_t[:, 2:], start[:, :2] / start[:, 2:], rtol=1e-6)
    # a hand with too few valid pixels, or nothing measured, keeps its bytes
    kept = DR.refine(render, verts, start, sensor, SCENE["unit"], min_pixels=10 ** 6)
    assert kept[0].tobytes() == start.tobytes() and not kept[3].any() and np.isfinite(kept[1]).all()
    blind = DR.refine(render, verts, start, np.zeros_like(sensor), SCENE["unit"])
    assert blind[0].tobytes() == start.tobytes() and not blind[3].any() and np.isnan(blind[1]).all() and (blind[2] == 0).all()


def test_refine_step_conditions():
    cam_t = np.array([[0.1, 0.2, 0.5]] * 5, np.float32)
    counts = np.zeros((5, 8), np.int64)
    counts[:, 0], counts[:, 5] = 1000, 400
    counts[2, 5] = 199                                                                  # too few pixels
    counts[3, 0] = 1601                                                                 # valid / covered just below a quarter
    median = np.array([0.1, np.nan, 0.1, 0.1, -0.46])                                   # the last lands in front of znear
    new, ok = DR.refine_step(cam_t, median, counts)
    assert ok.tolist() == [True, False, False, False, False] and new[1:].tobytes() == cam_t[1:].tobytes()
    assert new[0].tolist() == (cam_t[0].astype(np.float64) * ((np.float64(cam_t[0, 2]) + 0.1) / np.float64(cam_t[0, 2]))).astype(np.float32).tolist()
    counts[3, 0] = 1600
    assert DR.refine_step(cam_t, median, counts)[1].tolist() == [True, False, False, True, False]


# ------------------------------------------------------------------ surface
NAMES = ("hm_depth_residuals_workspace_bytes", "hm_depth_residuals")


def test_surface():
    header = open(os.path.join(ROOT, "include", "hamer_hip.h")).read()
    lib = L.load()
    for name in NAMES:
        assert re.search(r"\b%s\(" % name, header) and name in L.EXPORTS and hasattr(lib, name), name
    assert "depth_eval.hip" in B.SOURCES and os.path.exists(os.path.join(B.CSRC, "depth_eval.hip"))
    assert re.search(r"#define HM_VERSION 402\b", header) and L.HM_VERSION == 402 and lib.hm_version() == 402
    assert "contract(off)" in header and "LOWER median" in header
    src = open(os.path.join(B.CSRC, "depth_eval.hip")).read()
    assert "#pragma clang fp contract(off)" in src
    for word in ("getenv", "hipMalloc", "asm", "hipDeviceSynchronize", "hipStreamSynchronize", "printf"):
        assert word not in src, word
    assert lib.hm_depth_residuals_workspace_bytes.restype is C.c_size_t and len(lib.hm_depth_residuals.argtypes) == 22
    assert DE.COUNT_NAMES == DR.COUNT_NAMES


def test_workspace_bytes():
    lib = L.load()
    prev = 0
    for Q in (1, 2, 3, 16, 64, 256):
        n = lib.hm_depth_residuals_workspace_bytes(Q, 4096)
        assert n > prev and n % 8 == 0
        prev = n
    assert lib.hm_depth_residuals_workspace_bytes(0, 4096) > 0 and lib.hm_depth_residuals_workspace_bytes(1, 2) > 0
    for bad in ((-1, 64), (1, 0), (1, 1), (1, 63), (1, 4097), (1, 4098), (1, -2)):
        assert lib.hm_depth_residuals_workspace_bytes(*bad) == 0, bad


def _call(**kw):
    """hm_depth_residuals over MADE-UP device addresses that are never dereferenced: every case below must fail in the host
    part, before any launch."""
    a = dict(pred_depth=0x10000, pred_id=0x20000, sensor=0x30000, mask=0x40000, labels=0x50000, N=2, H=37, W=53, mesh_query=0x60000,
             n_meshes=5, Q=3, unit=0.001, raw_lo=1, raw_hi=65535, bin_m=0.0005, bins=4096, hist=0x70000, counts=0x80000, stats=0x90000,
             workspace=0xA0000, workspace_bytes=None, stream=None)
    a.update(kw)
    lib = L.load()
    if a["workspace_bytes"] is None:
        a["workspace_bytes"] = max(int(lib.hm_depth_residuals_workspace_bytes(max(a["Q"], 0), 4096)), 8)
    rc = lib.hm_depth_residuals(*[a[k] for k in ("pred_depth", "pred_id", "sensor", "mask", "labels", "N", "H", "W", "mesh_query",
                                                 "n_meshes", "Q", "unit", "raw_lo", "raw_hi", "bin_m", "bins", "hist", "counts", "stats",
                                                 "workspace", "workspace_bytes", "stream")])
    return rc, lib.hm_last_error_string().decode()


@pytest.mark.parametrize("kw,word", [
    (dict(pred_depth=None), "null"), (dict(pred_id=None), "null"), (dict(sensor=None), "null"), (dict(mesh_query=None), "null"),
    (dict(hist=None), "null"), (dict(counts=None), "null"), (dict(stats=None), "null"), (dict(workspace=None), "null"),
    (dict(N=0), "positive"), (dict(H=0), "positive"), (dict(W=-1), "positive"), (dict(N=1024, H=1024, W=2048), "2^31"),
    (dict(N=2, H=32768, W=32768), "2^31"), (dict(Q=-1), "negative"), (dict(n_meshes=-1), "negative"),
    (dict(bins=0), "bins"), (dict(bins=3), "bins"), (dict(bins=4095), "bins"), (dict(bins=4098), "bins"), (dict(bins=-2), "bins"),
    (dict(unit=0.0), "unit"), (dict(unit=-0.001), "unit"), (dict(unit=float("inf")), "unit"), (dict(unit=float("nan")), "unit"),
    (dict(bin_m=0.0), "bin_m"), (dict(bin_m=float("nan")), "bin_m"), (dict(bin_m=float("inf")), "bin_m"),
    (dict(raw_lo=10, raw_hi=9), "raw_lo"), (dict(workspace_bytes=0), "workspace"), (dict(workspace_bytes=3 * 8 - 1), "workspace"),
    (dict(counts=0x80004), "aligned"), (dict(stats=0x90004), "aligned"), (dict(hist=0x70002), "aligned"),
    (dict(workspace=0xA0002), "aligned"), (dict(pred_id=0x20002), "aligned"), (dict(pred_depth=0x10002), "aligned"),
    (dict(sensor=0x30001), "aligned"), (dict(labels=0x50002), "aligned"), (dict(mesh_query=0x60002), "aligned"),
])
def test_argument_checks(kw, word):
    rc, msg = _call(**kw)
    assert rc == -1 and "hm_depth_residuals" in msg and word in msg, (rc, msg)          # HM_ERR_ARG


def test_no_queries_pass_the_checks_without_a_launch():
    assert _call(Q=0)[0] == 0
    assert _call(Q=0, mesh_query=None, hist=None, counts=None, stats=None, workspace=None, workspace_bytes=0, mask=None, labels=None)[0] == 0
    assert L.load().hm_depth_residuals_workspace_bytes(3, 4096) == 3 * 8


# ------------------------------------------------------------------ the Python layer
def test_python_layer_raises_without_a_gpu_and_on_bad_inputs():
    d, i, s = torch.zeros(1, 4, 5), torch.zeros(1, 4, 5, dtype=torch.int32), torch.zeros(1, 4, 5, dtype=torch.int16)
    with pytest.raises(ValueError, match="GPU"):
        DE.depth_residuals(d, i, s, [0], 1)
    with pytest.raises(ValueError):
        DE.depth_residuals(d.numpy(), i.numpy(), s.numpy(), [0], 1)
    p = inspect.signature(DE.depth_residuals).parameters
    assert list(p) == ["pred_depth", "pred_id", "sensor", "mesh_query", "Q", "unit", "bin_m", "bins", "raw_range", "mask", "labels"]
    assert (p["unit"].default, p["bin_m"].default, p["bins"].default, p["raw_range"].default, p["mask"].default, p["labels"].default) \
        == (0.001, 0.0005, 4096, (1, 65535), None, None)
    assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(p)[5:])
    p = inspect.signature(DE.summary_from_hist).parameters
    assert list(p) == ["hist", "counts", "bin_m", "thresholds_m"] and p["thresholds_m"].default == (0.005, 0.010, 0.020)
    p = inspect.signature(DE.refine_cam_t).parameters
    assert list(p)[:8] == ["H", "W", "K", "vertices", "faces", "cam_t", "frame_index", "sensor"]
    assert (p["iterations"].default, p["min_pixels"].default, p["min_fraction"].default, p["znear"].default, p["mask"].default,
            p["labels"].default) == (2, 200, 0.25, 0.05, None, None) and p["unit"].default is inspect.Parameter.empty
    with pytest.raises(ValueError, match="GPU"):
        DE.refine_cam_t(4, 5, np.eye(3), torch.zeros(1, 3, 3), [[0, 1, 2]], torch.zeros(1, 3), [0], s, unit=0.001)
    ev = DE.DepthEvaluator()
    assert ev.n == 0 and ev.counts().shape == (0, 8) and ev.hist().shape == (0, 4096) and ev.per_query()["median"].shape == (0,)
    with pytest.raises(ValueError):
        ev.result()
    c = inspect.signature(DE.DepthEvaluator.__call__).parameters
    assert list(c)[:7] == ["self", "pred_depth", "pred_id", "sensor", "mesh_query", "Q", "sync"] and c["sync"].default is False
    import hamer_yolo_amd.hamer.utils as U
    assert U.__all__ == ["eval_pose", "Evaluator"]
    assert DE._ws == {} and DE.release_workspaces() is None


# ------------------------------------------------------------------ the drivers
def test_driver_parsers():
    from hamer_yolo_amd import d_infer, infer
    from hamer_yolo_amd import evaluate_depth as ED
    a = ED._parser().parse_args(["--pred", "A", "--depth-maps", "B", "--intrinsics", "K.txt"])
    assert (a.pred, a.depth_maps, a.intrinsics, a.depth_scale, a.masks, a.label, a.images, a.refine_to, a.json) == \
        ("A", "B", "K.txt", 0.001, None, 3, None, None, None)
    a = ED._parser().parse_args(["--pred", "A", "--depth-maps", "B", "--intrinsics", "K", "--depth-scale", "0.0001", "--masks", "M",
                                 "--label", "5", "--refine-to", "R", "--json", "o.json", "--images", "I"])
    assert (a.depth_scale, a.masks, a.label, a.refine_to, a.json, a.images) == (0.0001, "M", 5, "R", "o.json", "I")
    with pytest.raises(SystemExit):
        ED._parser().parse_args(["--pred", "A", "--depth-maps", "B"])                   # --intrinsics is required
    p = inspect.signature(ED.score_folder).parameters
    assert list(p)[:7] == ["npy_folder", "depth_folder", "hamer", "k_real", "unit", "mask_folder", "label"]
    assert (p["unit"].default, p["mask_folder"].default, p["label"].default, p["rank"].default, p["world"].default) == (0.001, None, 3, 0, 1)
    p = inspect.signature(ED.refine_folder).parameters
    assert list(p)[:5] == ["npy_folder", "depth_folder", "out_folder", "hamer", "k_real"] and p["rank"].default == 0 and p["world"].default == 1
    # the product drivers: opt-in, and a usage error without the real camera
    a = infer._parser().parse_args(["--input", "A", "--output", "B"])
    assert a.depth_maps is None and a.depth_scale == 0.001
    a = infer._parser().parse_args(["--input", "A", "--output", "B", "--depth-maps", "D", "--depth-scale", "0.0002", "--intrinsics", "K"])
    assert (a.depth_maps, a.depth_scale) == ("D", 0.0002)
    a = d_infer._parser().parse_args(["--input", "A", "--output", "B", "--intrinsics", "K", "--depth-maps", "D"])
    assert a.depth_maps == "D" and a.depth_scale == 0.001
    with pytest.raises(SystemExit) as e:
        infer.main(["--input", "A", "--output", "B", "--depth-maps", "D"])
    assert e.value.code == 2
    with pytest.raises(SystemExit) as e:
        infer.main(["--input", "A", "--output", "B", "--depth-scale", "0.01"])
    assert e.value.code == 2
    with pytest.raises(SystemExit):
        d_infer._parser().parse_args(["--input", "A", "--output", "B", "--depth-maps", "D"])
    with pytest.raises(ValueError, match="intrinsics"):
        ED.score_folder("A", "B", None, None)
    line = ED.format_line({"hands": 6, "scored": 5, "median_abs_mm": 3.25, "mean_abs_mm": 4.5, "inliers": {"5mm": 0.5, "10mm": 0.75},
                           "measured": 0.9, "occluded": 0.1, "n_skipped": 1})
    assert all(w in line for w in ("6 hands, 5 scored", "median |residual| 3.25 mm", "5mm 0.5000", "occluded 0.1000", "skipped 1"))


def test_depth_map_loading(tmp_path):
    from PIL import Image
    from hamer_yolo_amd import evaluate_depth as ED
    rng = np.random.default_rng(3)
    raw = rng.integers(0, 65536, (6, 7)).astype(np.uint16)
    raw[0, 0], raw[0, 1] = 0, 65535
    Image.fromarray(raw).save(tmp_path / "a.png")
    np.save(tmp_path / "b.npy", raw)
    np.save(tmp_path / "c.npy", raw.astype(np.float64) * 0.001)
    np.save(tmp_path / "d.npy", (raw.astype(np.float64) * 0.001).astype(np.float32))
    Image.fromarray(np.zeros((6, 7, 3), np.uint8)).save(tmp_path / "rgb.png")
    with Image.open(tmp_path / "a.png") as im:
        assert im.mode == "I;16"
    for name in ("a.png", "b.npy", "c.npy", "d.npy"):
        got = ED.load_depth(str(tmp_path / name), (6, 7), 0.001)
        assert got.dtype == np.uint16 and got.flags.c_contiguous and np.array_equal(got, raw), name
        assert ED.depth_size(str(tmp_path / name)) == (6, 7)
        assert ED.load_depth(str(tmp_path / name), (7, 6), 0.001) is None
    m = np.array([[np.nan, -1.0, 100.0, 0.0304]])
    np.save(tmp_path / "e.npy", m)
    assert ED.load_depth(str(tmp_path / "e.npy"), (1, 4), 0.001).tolist() == [[0, 0, 65535, 30]]
    assert ED.load_depth(str(tmp_path / "rgb.png"), (6, 7), 0.001) is None and ED.load_depth(str(tmp_path / "none.png"), (6, 7), 0.001) is None
    assert ED.find_depth(str(tmp_path), "a").endswith("a.png") and ED.find_depth(str(tmp_path), "b").endswith("b.npy")
    assert ED.find_depth(str(tmp_path), "zz") is None


def test_refined_record_keeps_existing_keys():
    from hamer_yolo_amd import evaluate_depth as ED
    hand = {"betas": np.arange(10, dtype=np.float32), "cam_t": np.array([0.1, 0.2, 0.5], np.float32), "is_right": True}
    data = {"right": hand, "left": dict(hand, is_right=False)}
    out = ED._refined_record(data, {"right": (np.array([0.12, 0.24, 0.6]), 0.1, 321, True), "left": (np.array([9.0, 9.0, 9.0]), 0.2, 12, False)})
    r, l = out["right"], out["left"]
    assert set(r) == set(hand) | set(ED.NEW_KEYS) and r["betas"] is hand["betas"]
    assert r["cam_t"].dtype == np.float32 and r["cam_t"].tolist() == np.array([0.12, 0.24, 0.6], np.float32).tolist()
    assert r["cam_t_unrefined"] is hand["cam_t"] and (r["depth_residual_m"], r["depth_pixels"], r["depth_refined"]) == (0.1, 321, True)
    assert l["cam_t"] is hand["cam_t"] and (l["depth_residual_m"], l["depth_pixels"], l["depth_refined"]) == (0.2, 12, False)
    assert hand.keys() == {"betas", "cam_t", "is_right"} and data["right"] is hand                   # the input is left alone
    none = ED._refined_record({"right": hand, "left": None}, {})
    assert none["left"] is None and none["right"]["cam_t"] is hand["cam_t"] and np.isnan(none["right"]["depth_residual_m"])
    assert none["right"]["depth_pixels"] == 0 and none["right"]["depth_refined"] is False
