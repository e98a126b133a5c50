"""Host checks of the depth fit (hm_depth_fit, hamer.utils.depth_eval.depth_fit / fit_rigid, evaluate_depth --refine-mode rigid):
the numpy rule of tests/depth_fit_rule.py against an independent least-squares build and against its own pixel-by-pixel form;
a map on which a fused multiply-subtract would change an integer; the rigid loop on renders of tests/zrender_rule.py; the folding
of a fit into a record; and the surface -- exports, header, build list, argument checks, the drivers' parsers.  No GPU."""
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
import depth_fit_rule as FR  # noqa: E402
import zrender_rule as ZR  # noqa: E402

from hamer_yolo_amd import build as B  # noqa: E402
from hamer_yolo_amd import lib as L  # noqa: E402
from hamer_yolo_amd.hamer.utils import depth_eval as DE  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_END_MM = 0.02          # the mean vertex error the rule's loop reaches on the 8-degree case on the CPU: 0.0195 mm measured


def blob_maps(seed, N=2, H=31, W=37):
    """Blobs of one id each on a smooth depth field (a pixel needs four neighbours of its id for a normal), a sensor a few
    millimetres off with holes, a label image; ids 0..3 and one past the table."""
    rng = np.random.default_rng(seed)
    n, v, u = np.meshgrid(np.arange(N), np.arange(H), np.arange(W), indexing="ij")
    z = 0.5 + 2e-4 * u - 1e-4 * v + 0.004 * np.sin(u / 6.0 + seed) * np.cos(v / 4.0) + 0.01 * n
    pid = np.full((N, H, W), -1, np.int32)
    pid[:, 2:14, 1:20], pid[:, 16:30, 3:18], pid[:, 0:15, 22:37], pid[:, 17:31, 20:36] = 0, 1, 2, 3
    pid[1, 20:26, 5:12] = 4
    depth = np.where(pid >= 0, z, 0.0).astype(np.float32)
    sensor = np.rint((z + 0.003 * np.sin(u / 9.0 + v / 7.0) + rng.normal(0, 0.0005, z.shape)) * 1000.0).astype(np.uint16)
    sensor[rng.random(z.shape) < 0.03] = 0
    sensor[0, 5:8, 5:8] += 60                                                           # beyond the gate
    depth[1, 8, 28] = np.nan
    mask = rng.choice(np.array([0, 3, 5], np.uint8), (N, H, W), p=[0.1, 0.6, 0.3])
    cams = np.array([[600.0, 610.0, 18.0, 15.0], [500.0, 480.0, 20.5, 13.25]])[:N]
    return depth, pid, sensor, mask, cams


PIVOT = np.array([[-0.002, 0.001, 0.5], [0.004, -0.003, 0.52], [0.0, 0.0, 1.3]])


# ------------------------------------------------------------------ the rule
def test_rule_against_brute_force():
    """Per used pixel an independent build: 3-D points from the depth map, np.cross, a NORMALISED normal, float sums."""
    for seed in (1, 2, 3):
        depth, pid, sensor, _, cams = blob_maps(seed)
        mq = np.array([0, 1, 0, -1])
        sums, counts, (idx, qs, _, _, _) = FR.fit(depth, pid, sensor, mq, 2, cams, PIVOT[:2], parts=True)
        N, H, W = pid.shape
        d = depth.astype(np.float64)

        def point(n, v, u):
            fx, fy, cx, cy = cams[n]
            return d[n, v, u] * np.array([(u - cx) / fx, (v - cy) / fy, 1.0])

        A, g, r2 = np.zeros((2, 6, 6)), np.zeros((2, 6)), np.zeros(2)
        for e, q in zip(idx, qs):
            n, v, u = np.unravel_index(e, pid.shape)
            nrm = np.cross(point(n, v, u + 1) - point(n, v, u - 1), point(n, v + 1, u) - point(n, v - 1, u))
            nrm = nrm / np.linalg.norm(nrm)
            p = point(n, v, u)
            s = p / d[n, v, u] * (float(sensor[n, v, u]) * 0.001)                       # the sensor's point on the same ray
            J = np.concatenate([np.cross(p - PIVOT[q], nrm), nrm])
            r = nrm @ (s - p)
            A[q] += np.outer(J, J); g[q] += J * r; r2[q] += r * r
        assert (counts[:, 6] >= 100).all() and counts[:, 6].sum() == len(idx)
        for q in range(2):
            M, gq = FR.matrix(sums[q], 0, 0.0, 1.0)
            bound = counts[q, 6] * 2.0 ** -31 + 1e-12 * counts[q, 6]                    # the quantisation, and the float sums' own error
            assert np.abs(M - A[q]).max() <= bound and np.abs(gq - g[q]).max() <= bound, (np.abs(M - A[q]).max(), bound)
            assert abs(float(sums[q, 27]) * 2.0 ** -30 - r2[q]) <= bound
            # the solve is the least-squares solution of the same damped system
            sol = FR.solve(sums[q:q + 1], counts[q:q + 1], 1e-3, 0.05, 50)[0]
            Md, _ = FR.matrix(sums[q], counts[q, 6], 1e-3, 0.05)
            assert sol[7] == 1.0 and np.allclose(sol[:6], np.linalg.solve(Md, gq), rtol=1e-9, atol=1e-15)
            assert sol[6] == np.sqrt(float(sums[q, 27]) * 2.0 ** -30 / counts[q, 6])


def test_rule_pixel_by_pixel():
    for seed, mq, Q in ((4, [0, 1, 2, 3], 4), (5, [0, 1, 0, -1, 2], 3), (6, [2, 2, 7, 1], 3)):
        depth, pid, sensor, mask, cams = blob_maps(seed)
        for kw in (dict(), dict(mask=mask, labels=[-2, -1, 3, 5][:Q]), dict(raw_range=(495, 530)), dict(gate_m=0.002, edge_m=0.0004),
                   dict(reach_m=0.012)):
            pv = np.concatenate([PIVOT, PIVOT[:1]])[:Q]
            a, b = FR.fit(depth, pid, sensor, mq, Q, cams, pv, **kw), FR.fit_loop(depth, pid, sensor, mq, Q, cams, pv, **kw)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), kw
            c = a[1]
            assert (c[:, 0] == c[:, 1:7].sum(1)).all() and (c[:, 7] == 0).all()
            if not kw:
                assert c[:, 3].sum() >= 9 and c[:, 2].sum() > 0 and c[:, 4].sum() > 0 and c[:, 6].max() >= 50
            if "reach_m" in kw:
                assert c[:, 5].sum() > 0
            if "mask" in kw:
                assert c[:, 1].sum() > 0
    # a pivot out of reach rejects a whole query; no pixel: rms NaN, not solved, zeros
    depth, pid, sensor, _, cams = blob_maps(7)
    sums, counts = FR.fit(depth, pid, sensor, [0, 1, 2], 3, cams, PIVOT)
    assert counts[2, 6] == 0 and counts[2, 5] > 100 and (sums[2] == 0).all()
    sol = FR.solve(sums, counts, 1e-3, 0.05, 50)
    assert sol[2].tolist()[:6] == [0.0] * 6 and np.isnan(sol[2, 6]) and sol[2, 7] == 0.0 and sol[:2, 7].tolist() == [1.0, 1.0]
    assert FR.solve(sums, counts, 1e-3, 0.05, 10 ** 6)[:, 7].tolist() == [0.0] * 3
    assert FR.COUNT_NAMES == DE.FIT_COUNT_NAMES


def test_contraction_would_show():
    depth, pid, sensor, cams, pv, unit, plain, fused = FR.contraction_case()
    print("llrint(rz * 2^30) per pixel: the rule", plain, "a fused multiply-subtract", fused)
    assert plain % 2 == 0 and abs(plain - fused) == 1
    sums, counts = FR.fit(depth, pid, sensor, [0], 1, cams, pv, unit=unit)
    used = int(counts[0, 6])
    assert used == 10 * 12 and sums[0, 26] == used * plain and sums[0, 20] == used * 2 ** 30
    loop = FR.fit_loop(depth, pid, sensor, [0], 1, cams, pv, unit=unit)
    assert np.array_equal(loop[0], sums) and np.array_equal(loop[1], counts)


def test_cholesky_order_and_singular():
    rng = np.random.default_rng(0)
    A = rng.normal(size=(6, 6))
    M, g = A @ A.T + 0.1 * np.eye(6), rng.normal(size=6)
    x, ok = FR.cholesky_solve(M, g)
    assert ok and np.allclose(x, np.linalg.solve(M, g), rtol=1e-10)
    M[2, :], M[:, 2] = 0.0, 0.0
    x, ok = FR.cholesky_solve(M, g)
    assert not ok
    # a flat fronto-parallel patch without damping is singular: in-plane motion is left to the damping
    depth, pid, sensor, cams, pv, unit, _, _ = FR.contraction_case()
    sums, counts = FR.fit(depth, pid, sensor, [0], 1, cams, pv, unit=unit)
    assert FR.solve(sums, counts, 0.0, 0.05, 50)[0].tolist()[:6] == [0.0] * 6 and FR.solve(sums, counts, 0.0, 0.05, 50)[0, 7] == 0.0
    sol = FR.solve(sums, counts, 1e-3, 0.05, 50)[0]
    assert sol[7] == 1.0 and abs(sol[5] - 0.003) < 1e-5 and np.abs(sol[3:5]).max() < 1e-12


# ------------------------------------------------------------------ the rigid loop on the rule's renders
SCENE = dict(H=240, W=320, K=np.array([[600.0, 0, 160.0], [0, 600.0, 120.0], [0, 0, 1.0]]), centre=np.array([0.03, -0.02, 0.5]),
             wall=1.5, unit=0.001, degrees=8.0, axis=(0.5, 0.7, 0.5), shift=(0.010, -0.008, 0.040))


@pytest.fixture(scope="module")
def ellipsoid_case():
    v, f = DR.ellipsoid()
    H, W, K, c = SCENE["H"], SCENE["W"], SCENE["K"], SCENE["centre"]

    def render(placed):
        meshes = [{"frame": j, "vertices": placed[j], "faces": f, "face_id0": j * len(f)} for j in range(len(placed))]
        r = ZR.render(len(placed), H, W, K, meshes)
        return r["depth"], r["mesh_id"]

    truth = (v + c)[None]
    sensor = DR.sensor_from_depth(render(truth.astype(np.float32))[0], SCENE["unit"], SCENE["wall"])
    axis = np.asarray(SCENE["axis"]) / np.linalg.norm(SCENE["axis"])
    verts = (v @ FR.exp_so3(axis * np.radians(SCENE["degrees"])).T)[None].astype(np.float32)
    start = (c + np.asarray(SCENE["shift"]))[None].astype(np.float32)
    return dict(render=render, truth=truth, sensor=sensor, verts=verts, start=start, cams=FR.cameras_of(K, 1))


def test_rigid_loop_on_the_ellipsoid(ellipsoid_case):
    s = ellipsoid_case

    def err(p):
        return float(np.linalg.norm(p - s["truth"], axis=2).mean() * 1e3)

    r = FR.fit_rigid(s["render"], s["verts"], s["start"], s["start"].astype(np.float64), s["sensor"], s["cams"], SCENE["unit"])
    trail = [err(p) for p in r["trail"]]
    print("mean vertex error in mm: start %.3f, after two ray rounds %.3f, after each rigid round" % (
        err(s["verts"].astype(np.float64) + s["start"][:, None]), trail[0]), ["%.4f" % e for e in trail[1:]],
        "rms %.3g m over %d pixels" % (r["rms"][0], r["used"][0]))
    assert all(b < a for a, b in zip(trail, trail[1:]))                                # the error falls every round
    assert trail[-1] < trail[0] and trail[0] > 5.0                                     # rigid ends below ray-only, which cannot do better
    assert trail[-1] <= 2 * HOST_END_MM
    assert r["updated"].all() and r["used"][0] > 10000 and r["rms"][0] < 0.0005 and r["cam_t"].dtype == np.float32
    # what is returned folds together: placed = rotation (vertices + ray cam_t - ray pivot) + pivot, cam_t = ray cam_t + shift
    ray = DR.refine(s["render"], s["verts"], s["start"], s["sensor"], SCENE["unit"])[0]
    placed0 = s["verts"].astype(np.float64) + ray.astype(np.float64)[:, None]
    again = np.einsum("bij,bvj->bvi", r["rotation"], placed0 - ray.astype(np.float64)[:, None]) + r["pivot"][:, None]
    assert np.abs(again - r["trail"][-1]).max() <= 1e-12
    assert np.abs(r["cam_t"].astype(np.float64) - r["pivot"]).max() <= 1e-7            # the pivot was the origin


def test_a_hand_that_stays_put(ellipsoid_case):
    s = ellipsoid_case
    args = (s["render"], s["verts"], s["start"], s["start"].astype(np.float64))
    eye = np.eye(3)[None]
    few = FR.fit_rigid(*args, s["sensor"], s["cams"], SCENE["unit"], iterations=2, min_pixels=10 ** 6, ray_kw=dict(min_pixels=10 ** 6))
    assert few["cam_t"].tobytes() == s["start"].tobytes() and few["rotation"].tobytes() == eye.tobytes() and not few["updated"].any()
    assert few["used"][0] == 0 or np.isfinite(few["rms"][0])
    blind = FR.fit_rigid(*args, np.zeros_like(s["sensor"]), s["cams"], SCENE["unit"], iterations=2)
    assert blind["cam_t"].tobytes() == s["start"].tobytes() and blind["rotation"].tobytes() == eye.tobytes() and not blind["updated"].any()
    assert blind["used"][0] == 0 and np.isnan(blind["rms"][0]) and blind["pivot"].tobytes() == s["start"].astype(np.float64).tobytes()
    capped = FR.fit_rigid(*args, s["sensor"], s["cams"], SCENE["unit"], ray_iterations=0, iterations=2, max_rot_rad=1e-9, gate_m=0.06)
    assert capped["cam_t"].tobytes() == s["start"].tobytes() and capped["rotation"].tobytes() == eye.tobytes() and capped["used"][0] > 1000
    capped = FR.fit_rigid(*args, s["sensor"], s["cams"], SCENE["unit"], ray_iterations=0, iterations=2, max_shift_m=1e-9, gate_m=0.06)
    assert capped["cam_t"].tobytes() == s["start"].tobytes() and not capped["updated"].any()


# ------------------------------------------------------------------ folding a fit into a record
def test_record_folding():
    from hamer_yolo_amd import evaluate_depth as ED
    rng = np.random.default_rng(11)
    X, J0 = rng.normal(0, 0.05, (40, 3)), np.array([0.09, 0.005, 0.006])                # a made-up hand and its wrist joint

    def mano(pose_global):                                                              # MANO turns the hand about the wrist joint
        return (X - J0) @ FR.exp_so3(pose_global).T + J0

    for is_right in (True, False):
        Mx = np.diag([1.0 if is_right else -1.0, 1.0, 1.0])
        pose, cam_t = rng.normal(0, 0.6, 3), np.array([0.1, -0.05, 0.6])
        w, t = rng.normal(0, 0.2, 3), rng.normal(0, 0.01, 3)
        R = FR.exp_so3(w)
        placed = mano(pose) @ Mx + cam_t
        pivot = Mx @ J0 + cam_t
        want = (placed - pivot) @ R.T + pivot + t                                       # the placed vertices, rotated directly
        new = ED.fold_rotation(pose, R, is_right)
        got = mano(new) @ Mx + (cam_t + t)
        assert np.abs(got - want).max() <= 1e-14, np.abs(got - want).max()
        assert np.abs(new - FR.fold(pose, cam_t, R, cam_t + t, is_right)[0]).max() <= 1e-14
        assert np.abs(ED.fold_rotation(pose, np.eye(3), is_right) - pose).max() <= 1e-14
    # near pi the logarithm still returns the rotation
    for w in (np.array([np.pi - 1e-9, 0, 0]), np.array([0.0, 2.0, 2.4]), np.array([1e-12, 0, 0])):
        assert np.abs(FR.exp_so3(ED._log_so3(FR.exp_so3(w))) - FR.exp_so3(w)).max() <= 1e-8
        assert np.abs(ED._exp_so3(w) - FR.exp_so3(w)).max() <= 1e-15
    # the record: existing keys kept, FIT_KEYS added, theta[:3] follows pose_global
    pg, ph = rng.normal(0, 0.3, 3).astype(np.float32), rng.normal(0, 0.1, 45).astype(np.float32)
    hand = {"betas": np.zeros(10, np.float32), "theta": np.concatenate([pg, ph]), "pose_hand": ph, "pose_global": pg,
            "cam_t": np.array([0.1, 0.2, 0.5], np.float32), "is_right": True}
    data = {"right": hand, "left": dict(hand, is_right=False)}
    R = FR.exp_so3(np.array([0.05, -0.02, 0.1]))
    out = ED._fitted_record(data, {"right": (np.array([0.12, 0.24, 0.6]), 0.1, 321, True), "left": (hand["cam_t"], 0.2, 12, False)},
                            {"right": (R, 0.0004, 5000, True), "left": (np.eye(3), float("nan"), 0, False)})
    r, l = out["right"], out["left"]
    assert set(r) == set(hand) | set(ED.NEW_KEYS) | set(ED.FIT_KEYS) and ED.NEW_KEYS == ("cam_t_unrefined", "depth_residual_m", "depth_pixels", "depth_refined")
    assert ED.FIT_KEYS == ("pose_global_unrefined", "depth_fit_rms_m", "depth_fit_pixels", "depth_fit")
    assert r["pose_global"].dtype == np.float32 and r["pose_global"].shape == (3,) and r["pose_global_unrefined"] is pg
    assert np.abs(r["pose_global"] - ED.fold_rotation(pg, R, True)).max() <= 1e-7
    assert r["theta"].dtype == np.float32 and np.array_equal(r["theta"][:3], r["pose_global"]) and np.array_equal(r["theta"][3:], ph)
    assert (r["depth_fit_rms_m"], r["depth_fit_pixels"], r["depth_fit"], r["depth_refined"]) == (0.0004, 5000, True, True)
    assert l["pose_global"] is pg and l["theta"] is hand["theta"] and l["cam_t"] is hand["cam_t"] and l["depth_fit"] is False
    assert np.isnan(l["depth_fit_rms_m"]) and l["depth_fit_pixels"] == 0
    assert np.array_equal(hand["theta"][:3], pg) and hand.keys() == {"betas", "theta", "pose_hand", "pose_global", "cam_t", "is_right"}
    none = ED._fitted_record({"right": hand, "left": None}, {}, {})
    assert none["left"] is None and none["right"]["pose_global"] is pg and none["right"]["depth_fit"] is False


# ------------------------------------------------------------------ surface
NAMES = ("hm_depth_fit_workspace_bytes", "hm_depth_fit")


def test_surface():
    header = open(os.path.join(ROOT, "include", "hamer_hip.h")).read()
    lib = L.load()
    for name in NAMES:
        assert re.search(r"\b%s\(" % name, header) and name in L.EXPORTS and hasattr(lib, name), name
    assert "depth_fit.hip" in B.SOURCES and os.path.exists(os.path.join(B.CSRC, "depth_fit.hip"))
    assert "---- Depth fit" in header and "llrint((J_i * J_j) / l2 * 2^30)" in header
    assert int(re.search(r"#define HM_VERSION (\d+)", header).group(1)) == L.HM_VERSION == lib.hm_version()
    src = open(os.path.join(B.CSRC, "depth_fit.hip")).read()
    assert "#pragma clang fp contract(off)" in src
    for word in ("getenv", "hipMalloc", "asm", "hipDeviceSynchronize", "hipStreamSynchronize", "printf"):
        assert word not in src, word
    assert lib.hm_depth_fit_workspace_bytes.restype is C.c_size_t and len(lib.hm_depth_fit.argtypes) == 28
    before = open(os.path.join(B.CSRC, "depth_eval.hip")).read()
    assert "hm_depth_fit" not in before                                                 # the residuals' unit is left alone


def test_workspace_bytes():
    lib = L.load()
    for Q in (1, 2, 3, 16, 64, 256, 100000):
        assert lib.hm_depth_fit_workspace_bytes(Q) == Q * 36 * 8
    assert lib.hm_depth_fit_workspace_bytes(0) == 36 * 8 and lib.hm_depth_fit_workspace_bytes(-1) == 0


ORDER = ("pred_depth", "pred_id", "sensor", "mask", "labels", "N", "H", "W", "mesh_query", "n_meshes", "Q", "cameras", "pivot", "unit",
         "raw_lo", "raw_hi", "gate_m", "edge_m", "reach_m", "damping", "lever_m", "min_pixels", "sums", "counts", "solution", "workspace",
         "workspace_bytes", "stream")


def _call(**kw):
    """hm_depth_fit over MADE-UP device addresses that are never dereferenced: every case below must fail in the host part,
    before any launch."""
    a = dict(pred_depth=0x10000, pred_id=0x20000, sensor=0x30000, mask=0x40000, labels=0x50000, N=2, H=37, W=53, mesh_query=0x60000,
             n_meshes=5, Q=3, cameras=0x70000, pivot=0x80000, unit=0.001, raw_lo=1, raw_hi=65535, gate_m=0.03, edge_m=0.005, reach_m=0.5,
             damping=1e-3, lever_m=0.05, min_pixels=200, sums=0x90000, counts=0xA0000, solution=0xB0000, workspace=0xC0000,
             workspace_bytes=None, stream=None)
    a.update(kw)
    lib = L.load()
    if a["workspace_bytes"] is None:
        a["workspace_bytes"] = max(int(lib.hm_depth_fit_workspace_bytes(max(a["Q"], 0))), 8)
    rc = lib.hm_depth_fit(*[a[k] for k in ORDER])
    return rc, lib.hm_last_error_string().decode()


INF, NAN = float("inf"), float("nan")


@pytest.mark.parametrize("kw,word", [
    (dict(pred_depth=None), "null"), (dict(pred_id=None), "null"), (dict(sensor=None), "null"), (dict(mesh_query=None), "null"),
    (dict(cameras=None), "null"), (dict(pivot=None), "null"), (dict(sums=None), "null"), (dict(counts=None), "null"),
    (dict(solution=None), "null"), (dict(workspace=None), "null"),
    (dict(N=0), "positive"), (dict(H=0), "positive"), (dict(W=-1), "positive"), (dict(N=1024, H=1024, W=2048), "2^31"),
    (dict(N=2, H=32768, W=32768), "2^31"), (dict(Q=-1), "negative"), (dict(n_meshes=-1), "negative"),
    (dict(unit=0.0), "unit"), (dict(unit=-0.001), "unit"), (dict(unit=INF), "unit"), (dict(unit=NAN), "unit"),
    (dict(raw_lo=10, raw_hi=9), "raw_lo"),
    (dict(gate_m=0.0), "gate_m"), (dict(gate_m=-0.01), "gate_m"), (dict(gate_m=0.2500001), "gate_m"), (dict(gate_m=NAN), "gate_m"),
    (dict(edge_m=0.0), "edge_m"), (dict(edge_m=-1.0), "edge_m"), (dict(edge_m=INF), "edge_m"), (dict(edge_m=NAN), "edge_m"),
    (dict(reach_m=0.0), "reach_m"), (dict(reach_m=1.0000001), "reach_m"), (dict(reach_m=NAN), "reach_m"),
    (dict(damping=-1e-9), "damping"), (dict(damping=INF), "damping"), (dict(damping=NAN), "damping"),
    (dict(lever_m=0.0), "lever_m"), (dict(lever_m=-0.05), "lever_m"), (dict(lever_m=INF), "lever_m"), (dict(lever_m=NAN), "lever_m"),
    (dict(min_pixels=0), "min_pixels"), (dict(min_pixels=-5), "min_pixels"),
    (dict(workspace_bytes=0), "workspace"), (dict(workspace_bytes=3 * 36 * 8 - 1), "workspace"),
    (dict(sums=0x90004), "aligned"), (dict(counts=0xA0004), "aligned"), (dict(solution=0xB0004), "aligned"),
    (dict(workspace=0xC0004), "aligned"), (dict(cameras=0x70004), "aligned"), (dict(pivot=0x80004), "aligned"),
    (dict(pred_id=0x20002), "aligned"), (dict(pred_depth=0x10002), "aligned"), (dict(sensor=0x30001), "aligned"),
    (dict(labels=0x50002), "aligned"), (dict(mesh_query=0x60002), "aligned"),
])
def test_argument_checks(kw, word):
    rc, msg = _call(**kw)
    assert rc == -1 and "hm_depth_fit" in msg and word in msg, (rc, msg)                # HM_ERR_ARG


def test_no_queries_and_limits_pass_the_checks_without_a_launch():
    assert _call(Q=0)[0] == 0
    assert _call(Q=0, mesh_query=None, cameras=None, pivot=None, sums=None, counts=None, solution=None, workspace=None,
                 workspace_bytes=0, mask=None, labels=None)[0] == 0
    assert _call(Q=0, gate_m=0.25, reach_m=1.0, damping=0.0, min_pixels=1)[0] == 0      # the ends of the ranges are legal


# ------------------------------------------------------------------ the Python layer and the drivers
def test_python_layer_raises_without_a_gpu_and_on_bad_inputs():
    d, i, s = torch.zeros(1, 4, 5), torch.zeros(1, 4, 5, dtype=torch.int32), torch.zeros(1, 4, 5, dtype=torch.int16)
    pv = torch.zeros(1, 3, dtype=torch.float64)
    with pytest.raises(ValueError, match="GPU"):
        DE.depth_fit(d, i, s, [0], 1, np.eye(3), pv, unit=0.001)
    with pytest.raises(ValueError):
        DE.depth_fit(d.numpy(), i.numpy(), s.numpy(), [0], 1, np.eye(3), pv, unit=0.001)
    p = inspect.signature(DE.depth_fit).parameters
    assert list(p) == ["pred_depth", "pred_id", "sensor", "mesh_query", "Q", "K", "pivot", "unit", "gate_m", "edge_m", "reach_m", "damping",
                       "lever_m", "min_pixels", "raw_range", "mask", "labels"]
    assert p["unit"].default is inspect.Parameter.empty and all(p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(p)[7:])
    assert tuple(p[k].default for k in list(p)[8:]) == (0.03, 0.005, 0.5, 1e-3, 0.05, 200, (1, 65535), None, None)
    p = inspect.signature(DE.fit_rigid).parameters
    assert list(p)[:9] == ["H", "W", "K", "vertices", "faces", "cam_t", "pivot", "frame_index", "sensor"]
    assert (p["ray_iterations"].default, p["iterations"].default, p["max_rot_rad"].default, p["max_shift_m"].default) == (2, 6, 0.5, 0.1)
    assert p["unit"].default is inspect.Parameter.empty and p["unit"].kind is inspect.Parameter.KEYWORD_ONLY
    with pytest.raises(ValueError, match="GPU"):
        DE.fit_rigid(4, 5, np.eye(3), torch.zeros(1, 3, 3), [[0, 1, 2]], torch.zeros(1, 3), torch.zeros(1, 3), [0], s, unit=0.001)
    w = torch.tensor([[0.3, -0.2, 0.5], [0.0, 0.0, 0.0], [1e-10, 0.0, 0.0]], dtype=torch.float64)
    assert np.abs(DE.exp_so3(w).numpy() - FR.exp_so3(w.numpy())).max() <= 1e-15
    cams = DE._cameras(np.array([[600.0, 0, 160.0], [0, 610.0, 120.0], [0, 0, 1.0]]), 2, torch.device("cpu"))
    assert cams.tolist() == [[600.0, 610.0, 160.0, 120.0]] * 2 and cams.dtype == torch.float64 and cams.is_contiguous()
    assert DE._fit_ws == {} and DE.release_fit_workspaces() is None


def test_driver_parsers():
    from hamer_yolo_amd import d_infer, infer
    from hamer_yolo_amd import evaluate_depth as ED
    a = ED._parser().parse_args(["--pred", "A", "--depth-maps", "B", "--intrinsics", "K.txt"])
    assert a.refine_mode == "ray" and a.refine_to is None
    a = ED._parser().parse_args(["--pred", "A", "--depth-maps", "B", "--intrinsics", "K", "--refine-to", "R", "--refine-mode", "rigid"])
    assert (a.refine_to, a.refine_mode) == ("R", "rigid")
    with pytest.raises(SystemExit):
        ED._parser().parse_args(["--pred", "A", "--depth-maps", "B", "--intrinsics", "K", "--refine-mode", "affine"])
    p = inspect.signature(ED.refine_folder).parameters
    assert p["mode"].default == "ray" and p["fit_iterations"].default == 6 and p["iterations"].default == 2
    assert list(p)[:5] == ["npy_folder", "depth_folder", "out_folder", "hamer", "k_real"]
    with pytest.raises(ValueError, match="mode"):
        ED.refine_folder("A", "B", "C", None, np.eye(3), mode="affine")
    a = infer._parser().parse_args(["--input", "A", "--output", "B"])
    assert a.depth_fit == "ray" and a.depth_maps is None and a.depth_scale == 0.001
    a = infer._parser().parse_args(["--input", "A", "--output", "B", "--depth-maps", "D", "--intrinsics", "K", "--depth-fit", "rigid"])
    assert (a.depth_maps, a.depth_fit) == ("D", "rigid")
    a = d_infer._parser().parse_args(["--input", "A", "--output", "B", "--intrinsics", "K", "--depth-maps", "D", "--depth-fit", "rigid"])
    assert a.depth_fit == "rigid"
    assert d_infer._parser().parse_args(["--input", "A", "--output", "B", "--intrinsics", "K"]).depth_fit == "ray"
    with pytest.raises(SystemExit) as e:
        infer.main(["--input", "A", "--output", "B", "--depth-fit", "rigid"])          # needs --depth-maps
    assert e.value.code == 2
    with pytest.raises(SystemExit):
        infer._parser().parse_args(["--input", "A", "--output", "B", "--depth-fit", "affine"])
