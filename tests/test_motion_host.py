"""The motion rule (tests/motion_rule.py, the numpy statement of include/hamer_hip.h "Motion") against independent mathematics,
and the host code of hamer/utils/motion.py, evaluate_motion.py and the --smooth-* flags.  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import motion_rule as MR  # noqa: E402

from hamer_yolo_amd.hamer.utils import motion as MO  # noqa: E402


# ------------------------------------------------------------------ helpers (scipy-free rotations, used by the GPU tests too)
def rotmat(v):
    """Rodrigues in fp64: axis-angle (..., 3) -> (..., 3, 3)."""
    v = np.asarray(v, np.float64)
    th = np.linalg.norm(v, axis=-1)[..., None, None]
    k = v / np.maximum(np.linalg.norm(v, axis=-1, keepdims=True), 1e-300)
    K = np.zeros(v.shape[:-1] + (3, 3))
    K[..., 0, 1], K[..., 0, 2], K[..., 1, 0] = -k[..., 2], k[..., 1], k[..., 2]
    K[..., 1, 2], K[..., 2, 0], K[..., 2, 1] = -k[..., 0], -k[..., 1], k[..., 0]
    return np.eye(3) + np.sin(th) * K + (1.0 - np.cos(th)) * (K @ K)


def angle_deg(a, b):
    """The angle between rotations a and b (..., 3, 3) in degrees."""
    c = (np.einsum("...ij,...ij->...", a, b) - 1.0) * 0.5
    return np.degrees(np.arccos(np.clip(c, -1.0, 1.0)))


def random_rotations(rng, shape, spread_deg):
    """Rotations within ``spread_deg`` of a random base rotation per leading index (the last axis of shape varies about it)."""
    base = rotmat(rng.normal(size=shape[:-1] + (1, 3)) * 2.0)
    axis = rng.normal(size=shape + (3,))
    axis /= np.linalg.norm(axis, axis=-1, keepdims=True)
    return base @ rotmat(axis * np.radians(spread_deg) * rng.uniform(0.0, 1.0, shape + (1,)))


def svd_project(m):
    u, _, vt = np.linalg.svd(m)
    d = np.sign(np.linalg.det(u @ vt))
    u[..., :, 2] *= d[..., None]
    return u @ vt


def constant_velocity(N, S, J, C, rng, deg_per_frame=6.9):
    axis = rng.normal(size=(S, J, 3))
    axis /= np.linalg.norm(axis, axis=-1, keepdims=True)
    t = np.arange(N, dtype=np.float64)[:, None, None, None]
    rot = rotmat(rng.normal(size=(1, S, J, 3))) @ rotmat(axis[None] * np.radians(deg_per_frame) * t)
    lin = rng.normal(size=(1, S, C)) + rng.normal(size=(1, S, C)) * t[:, :, :, 0]
    return rot, lin


# ------------------------------------------------------------------ the rule
@pytest.mark.parametrize("spread", [10, 40, 80, 120, 160])
def test_polar_iteration_lands_on_the_svd_projection(spread):
    rng = np.random.default_rng(spread)
    w = MR.window_weights(4, 2.0)
    ws = np.concatenate([w[:0:-1], w])                                   # the 9 samples of a full window
    r = random_rotations(rng, (200, 9), spread)
    m = np.einsum("k,nkij->nij", ws, r) / ws.sum()
    x, bad = MR.polar(m)
    assert bad.mean() <= 0.5 and (~bad).sum() > 0                        # the rule keeps some, at 160 degrees too
    err = np.abs(x[~bad] - svd_project(m[~bad])).max()
    print(f"spread {spread}: {int((~bad).sum())} kept, max |rule - svd| {err:.3g}")
    assert err < 1e-12
    assert np.abs(np.linalg.det(x[~bad]) - 1.0).max() < 1e-12


def test_constant_velocity_passes_through_for_any_presence():
    rng = np.random.default_rng(3)
    N, S, J, C = 60, 2, 16, 13
    rot, lin = constant_velocity(N, S, J, C, rng)
    present = (rng.uniform(size=(N, S)) > 0.25).astype(np.uint8)
    r = MR.track_smooth(rot, lin, present, MR.window_weights(6, 2.0))
    here = present != 0
    filled = r["status"] == MR.FILLED
    assert np.array_equal(filled, ~here & (r["pairs"] > 0)) and filled.sum() >= 5
    assert not (r["status"] == MR.DEGENERATE).any()
    ok = np.isin(r["status"], (MR.KEPT, MR.SMOOTHED, MR.FILLED))
    assert np.abs(r["rot"][ok] - rot[ok]).max() < 1e-12
    assert np.abs(r["lin"][ok] - lin[ok]).max() < 1e-12 * max(1.0, np.abs(lin).max())
    assert np.isnan(r["rot"][r["status"] == MR.ABSENT]).all() and np.isnan(r["lin"][r["status"] == MR.ABSENT]).all()
    assert np.array_equal(r["status"] == MR.ABSENT, ~here & (r["pairs"] == 0))
    # both ends of the sequence: a present end frame has no pair and keeps its bytes
    for t in (0, N - 1):
        for s in range(S):
            if here[t, s]:
                assert r["status"][t, s] == MR.KEPT and r["rot"][t, s].tobytes() == rot[t, s].tobytes()


def test_opposite_rotations_around_a_missing_centre_are_degenerate():
    rot = np.tile(np.eye(3), (3, 1, 2, 1, 1))
    rot[2, 0, 1] = rotmat([0.0, 0.0, np.pi])                             # joint 1: 180 degrees apart across the gap
    lin = np.arange(3.0).reshape(3, 1, 1)
    r = MR.track_smooth(rot, lin, np.array([[1], [0], [1]], np.uint8), MR.window_weights(1, 2.0))
    assert r["status"][:, 0].tolist() == [MR.KEPT, MR.DEGENERATE, MR.KEPT]
    assert np.isnan(r["rot"][1]).all() and np.isnan(r["lin"][1]).all() and np.isnan(r["moved"]).all()
    assert r["pairs"][:, 0].tolist() == [0, 1, 0] and r["nearest_pair"][:, 0].tolist() == [0, 1, 0]
    # the same with the centre present: the whole hand keeps its bytes, the joint that could be averaged included
    r = MR.track_smooth(rot, lin, np.ones((3, 1), np.uint8), np.array([0.0, 1.0]))
    assert r["status"][1, 0] == MR.DEGENERATE and r["rot"][1].tobytes() == rot[1].tobytes() and r["lin"][1, 0, 0] == 1.0


def test_radius_zero_keeps_every_byte():
    rng = np.random.default_rng(5)
    rot, lin = constant_velocity(7, 2, 3, 4, rng)
    rot[2, 0, 0, 0, 0] = np.float64("nan")
    present = np.ones((7, 2), np.uint8)
    present[4, 1] = 0
    r = MR.track_smooth(rot, lin, present, MR.window_weights(0, 2.0))
    here = present != 0
    assert (r["status"][here] == MR.KEPT).all() and r["status"][4, 1] == MR.ABSENT
    assert r["rot"][here].tobytes() == rot[here].tobytes() and r["lin"][here].tobytes() == lin[here].tobytes()
    assert not r["pairs"].any() and not r["nearest_pair"].any() and np.isnan(r["moved"]).all()


def noisy_track(N=80, seed=11, deg_per_frame=5.0, noise_deg=4.0):
    rng = np.random.default_rng(seed)
    clean, lin = constant_velocity(N, 1, 16, 13, rng, deg_per_frame)
    # a slowly changing rate keeps it a motion rather than a line: still at most 7 degrees per frame
    bend = rotmat(np.array([0.0, 0.0, 1.0]) * np.radians(2.0) * np.sin(np.arange(N) / 9.0)[:, None, None, None] * 9.0)
    clean = clean @ bend
    noise = rng.normal(size=(N, 1, 16, 3))
    noise *= np.radians(noise_deg) / np.sqrt(3.0)
    return clean, clean @ rotmat(noise), lin, lin + rng.normal(size=lin.shape) * 0.004


def rot_accel_deg(r):
    """Angle of the second difference R[t-1]^T R[t] against R[t]^T R[t+1], degrees per frame^2."""
    step = np.swapaxes(r[:-1], -1, -2) @ r[1:]
    return angle_deg(step[:-1], step[1:])


def test_smoothing_lowers_acceleration_and_error_of_a_noisy_track():
    clean, noisy, lin, lin_noisy = noisy_track()
    assert angle_deg(clean[:-1], clean[1:]).max() <= 7.0
    r = MR.track_smooth(noisy, lin_noisy, np.ones((len(noisy), 1), np.uint8), MR.window_weights(6, 2.0))
    assert not (r["status"] == MR.DEGENERATE).any()
    before, after = rot_accel_deg(noisy).mean(), rot_accel_deg(r["rot"]).mean()
    e0, e1 = angle_deg(noisy, clean).mean(), angle_deg(r["rot"], clean).mean()
    print(f"acceleration {before:.2f} -> {after:.2f} deg/frame^2, error {e0:.2f} -> {e1:.2f} deg")
    assert after < before and e1 < e0
    assert np.abs(r["lin"] - lin)[1:-1].mean() < np.abs(lin_noisy - lin)[1:-1].mean()
    # moved is the squared Frobenius distance: the angle it stands for is the angle between input and output
    s = r["status"][:, 0] == MR.SMOOTHED
    assert np.allclose(MO.moved_degrees(r["moved"][s]), angle_deg(noisy[s], r["rot"][s]), atol=1e-6)


def test_jitter_rule_is_the_second_difference():
    rng = np.random.default_rng(2)
    N, S, P = 9, 2, 70
    a, b, c = rng.normal(size=(3, 1, S, P, 3))
    t = np.arange(N, dtype=np.float64)[:, None, None, None]
    x = a * t * t + b * t + c
    present = np.ones((N, S), np.uint8)
    present[4, 1] = 0
    acc = MR.track_jitter(x, present)
    want = np.linalg.norm(2.0 * a, axis=-1).mean(-1)[0]
    assert np.isnan(acc[[0, -1]]).all() and np.isnan(acc[3:6, 1]).all() and np.isfinite(acc[1:-1, 0]).all()
    assert np.allclose(acc[1:-1, 0], want[0], rtol=1e-9) and np.allclose(acc[[1, 2, 6, 7], 1], want[1], rtol=1e-9)
    assert np.isnan(MR.track_jitter(x[:2], present[:2])).all()


def test_window_weights():
    w = MO.window_weights(4, 2.0)
    assert w.dtype == np.float64 and w[0] == 1.0 and w.tobytes() == MR.window_weights(4, 2.0).tobytes()
    assert np.allclose(w[1:], np.exp(-0.5 * (np.arange(1, 5) / 2.0) ** 2)) and len(MO.window_weights(0, 1.0)) == 1
    for bad in ((33, 2.0), (-1, 2.0), (4, 0.0), (4, float("nan")), (2.5, 2.0)):
        with pytest.raises(ValueError):
            MO.window_weights(*bad)
    assert MO.STATUSES == ("KEPT", "SMOOTHED", "FILLED", "ABSENT", "DEGENERATE")
    assert [getattr(MR, n) for n in MO.STATUSES] == [0, 1, 2, 3, 4] == [getattr(MO, n) for n in MO.STATUSES]


def test_status_names_match_the_header():
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "hamer_hip.h")).read()
    for i, n in enumerate(MO.STATUSES):
        assert re.search(rf"HM_TRACK_{n} = {i}\b", hdr)
    assert "#define HM_MOTION_MAX_RADIUS 32" in hdr and "#define HM_MOTION_MAX_POINTS 1024" in hdr
    assert MO.MAX_RADIUS == MR.MAX_RADIUS == 32 and MO.MAX_POINTS == 1024


# ------------------------------------------------------------------ host code
def test_natural_key_orders_digit_runs_as_integers():
    stems = ["frame_10", "frame_2", "frame_1", "f_2_b", "f_2_a", "f_10_a", "10", "9", "frame_02"]
    got = sorted(stems, key=MO.natural_key)
    assert got == ["9", "10", "f_2_a", "f_2_b", "f_10_a", "frame_1", "frame_2", "frame_02", "frame_10"] or \
        got == ["9", "10", "f_2_a", "f_2_b", "f_10_a", "frame_1", "frame_02", "frame_2", "frame_10"]
    assert sorted([f"f_{i}" for i in range(1, 25)], key=MO.natural_key) == [f"f_{i}" for i in range(1, 25)]
    assert sorted(["a", "1"], key=MO.natural_key) == ["1", "a"]         # digits and text never compare with each other


def hand(rng, is_right, cam_shape=(3,), dtype=np.float32):
    pg, ph = rng.normal(size=3) * 0.5, rng.normal(size=45) * 0.3
    return {"betas": rng.normal(size=10).astype(dtype), "theta": np.concatenate([pg, ph]).astype(dtype), "pose_hand": ph.astype(dtype),
            "pose_global": pg.astype(dtype), "cam_t": (rng.normal(size=3) * 0.1 + [0, 0, 0.5]).reshape(cam_shape).astype(dtype),
            "is_right": is_right}


def test_sequence_tracks_round_trip():
    rng = np.random.default_rng(8)
    recs = [{"right": hand(rng, True), "left": None}, {"right": None, "left": hand(rng, False, (1, 3))},
            {"right": hand(rng, True, (1, 3), np.float64), "left": hand(rng, False)}, {"right": None, "left": None}]
    tr = MO.sequence_tracks(recs)
    assert tr["present"].tolist() == [[1, 0], [0, 1], [1, 1], [0, 0]] and tr["present"].dtype == np.uint8
    assert tr["axis_angle"].shape == (4, 2, 16, 3) and tr["lin"].shape == (4, 2, 13) and tr["lin"].dtype == np.float64
    assert not tr["axis_angle"][3].any() and not tr["lin"][0, 1].any()
    for t, rec in enumerate(recs):
        for s, side in enumerate(MO.SIDES):
            h = rec[side]
            if h is None:
                continue
            back = MO.track_hand(tr["axis_angle"][t, s], tr["lin"][t, s], like=h)
            assert set(back) == set(MO.POSE_KEYS)
            for k in MO.POSE_KEYS:
                assert back[k].dtype == h[k].dtype and back[k].shape == h[k].shape and back[k].tobytes() == h[k].tobytes(), k
    plain = MO.track_hand(tr["axis_angle"][0, 0], tr["lin"][0, 0])
    assert {k: (v.shape, v.dtype) for k, v in plain.items()} == {
        "pose_global": ((3,), np.float32), "pose_hand": ((45,), np.float32), "theta": ((48,), np.float32), "betas": ((10,), np.float32),
        "cam_t": ((3,), np.float32)}


def test_summary():
    a = np.array([[0.001, np.nan], [0.003, 0.002], [np.nan, np.nan]])
    s = MO.summary(a, fps=30.0)
    assert s["n"] == 3 and s["mean"] == pytest.approx(2.0) and s["median"] == pytest.approx(2.0) and s["max"] == pytest.approx(3.0)
    assert s["p95"] == pytest.approx(np.percentile([1.0, 3.0, 2.0], 95)) and s["mean_m_s2"] == pytest.approx(0.002 * 900.0)
    e = MO.summary(np.full((2, 2), np.nan))
    assert e["n"] == 0 and np.isnan(e["mean"]) and "mean_m_s2" not in e


class _Stub:
    device = "cpu"


def stub_smooth(tracks, device, radius=4, sigma=2.0):
    """``smooth_tracks`` without a GPU: the rule on host matrices."""
    from hamer_yolo_amd.infer import rodrigues_log_batch
    N = len(tracks["present"])
    r = MR.track_smooth(rotmat(tracks["axis_angle"]), tracks["lin"], tracks["present"], MR.window_weights(radius, sigma))
    aa = rodrigues_log_batch(np.nan_to_num(r["rot"]).reshape(-1, 3, 3)).reshape(N, 2, 16, 3)
    return {"status": r["status"], "pairs": r["pairs"], "nearest_pair": r["nearest_pair"],
            "moved_deg": MO.moved_degrees(r["moved"]).astype(np.float32), "axis_angle": aa, "lin": r["lin"]}


def test_smooth_folder_folds_the_records(tmp_path, monkeypatch):
    from hamer_yolo_amd import evaluate_motion as EM
    monkeypatch.setattr(MO, "smooth_tracks", stub_smooth)
    rng = np.random.default_rng(4)
    src, out = tmp_path / "in", tmp_path / "out"
    src.mkdir()
    recs = {}
    for i in range(1, 13):
        right = None if i in (5, 9, 10) else hand(rng, True, (1, 3) if i % 2 else (3,))
        if right is not None:
            right["visible_share"] = 0.5                                  # a per-frame measurement
        recs[f"f_{i}"] = {"right": right, "left": hand(rng, False, dtype=np.float64) if i == 3 else None}
        np.save(src / f"f_{i}.npy", recs[f"f_{i}"])
    assert [s for s, _, _ in EM.load_sequence(str(src))] == [f"f_{i}" for i in range(1, 13)]
    res = EM.smooth_folder(str(src), str(out), _Stub(), radius=1, sigma=2.0, max_fill=1)
    got = {s: rec for s, _, rec in EM.load_sequence(str(out))}
    # f_5 has both neighbours and is filled; f_9 and f_10 have no pair at radius 1; f_1 and f_12 are ends: KEPT
    f5 = got["f_5"]["right"]
    assert set(f5) == set(MO.POSE_KEYS) | {"is_right", "track_status", "track_pairs", "track_filled"}
    assert f5["is_right"] is True and f5["track_filled"] is True and f5["track_status"] == "FILLED" and f5["track_pairs"] == 1
    assert all(f5[k].dtype == np.float32 for k in MO.POSE_KEYS) and f5["theta"].shape == (48,) and f5["cam_t"].shape == (3,)
    assert np.array_equal(f5["theta"], np.concatenate([f5["pose_global"], f5["pose_hand"]]))
    mid = (recs["f_4"]["right"]["cam_t"].reshape(3).astype(np.float64) + recs["f_6"]["right"]["cam_t"].reshape(3)) / 2
    assert np.allclose(f5["cam_t"], mid, atol=1e-6)
    assert got["f_9"]["right"] is None and got["f_10"]["right"] is None
    for stem in ("f_1", "f_12", "f_4", "f_6", "f_8", "f_11"):             # no pair: next to a gap, or at an end
        a, b = got[stem]["right"], recs[stem]["right"]
        assert set(a) == set(b) | {"track_status", "track_pairs"} and a["track_status"] == "KEPT" and a["track_pairs"] == 0
        assert all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() and np.asarray(a[k]).dtype == np.asarray(b[k]).dtype for k in b)
    lone = got["f_3"]["left"]
    assert lone["track_status"] == "KEPT" and lone["cam_t"].dtype == np.float64
    for stem in ("f_2", "f_3", "f_7"):
        a, b = got[stem]["right"], recs[stem]["right"]
        assert a["track_status"] == "SMOOTHED" and a["track_pairs"] == 1 and a["visible_share"] == 0.5
        assert set(a) == set(b) | {"track_status", "track_pairs", "track_moved_deg", "pose_global_unsmoothed", "pose_hand_unsmoothed",
                                   "betas_unsmoothed", "cam_t_unsmoothed"}
        assert a["track_moved_deg"].shape == (16,) and a["track_moved_deg"].dtype == np.float32 and (a["track_moved_deg"] > 0).all()
        for k in MO.POSE_KEYS:
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and not np.array_equal(a[k], b[k]), k
        for k in ("pose_global", "pose_hand", "betas", "cam_t"):
            assert a[k + "_unsmoothed"].tobytes() == b[k].tobytes()
        assert np.array_equal(a["theta"], np.concatenate([a["pose_global"].reshape(-1), a["pose_hand"].reshape(-1)]))
    assert res == {"records": 12, "smoothed": 3, "filled": 1, "kept": 7, "degenerate": 0, "max_moved_deg": res["max_moved_deg"],
                   "max_moved_stem": res["max_moved_stem"]}
    assert res["max_moved_stem"] in ("f_2", "f_3", "f_7") and res["max_moved_deg"] > 0
    # max_fill 0 never fills; in place gives the bytes of the second folder
    none = EM.smooth_folder(str(src), str(tmp_path / "nofill"), _Stub(), radius=1, sigma=2.0, max_fill=0)
    assert none["filled"] == 0 and np.load(tmp_path / "nofill" / "f_5.npy", allow_pickle=True).item()["right"] is None
    EM.smooth_folder(str(src), str(src), _Stub(), radius=1, sigma=2.0, max_fill=1)
    for i in range(1, 13):
        assert open(src / f"f_{i}.npy", "rb").read() == open(out / f"f_{i}.npy", "rb").read()


def test_degenerate_hand_keeps_its_bytes_in_the_record():
    rng = np.random.default_rng(6)
    h = hand(rng, True)
    out = MO.fold_hand(h, True, MO.DEGENERATE, 2, 1, np.zeros((16, 3)), np.zeros(13), np.full(16, np.nan))
    assert set(out) == set(h) | {"track_status", "track_pairs"} and out["track_status"] == "DEGENERATE" and out["track_pairs"] == 2
    assert all(out[k] is h[k] for k in h)
    assert MO.fold_hand(None, False, MO.FILLED, 1, 3, np.zeros((16, 3)), np.zeros(13), None, max_fill=2) is None
    assert MO.fold_hand(None, False, MO.ABSENT, 0, 0, np.zeros((16, 3)), np.zeros(13), None) is None
    f = MO.fold_hand(None, False, MO.FILLED, 1, 2, np.zeros((16, 3)), np.zeros(13), None, max_fill=2)
    assert f["is_right"] is False and f["track_filled"] is True


# ------------------------------------------------------------------ usage errors
def usage_error(fn, argv, capsys, text):
    with pytest.raises(SystemExit) as e:
        fn(argv)
    assert e.value.code == 2 and text in capsys.readouterr().err


def test_smooth_flags_give_usage_errors(capsys):
    from hamer_yolo_amd import d_infer, infer
    base = ["--input", "A", "--output", "B"]
    for flag, v in (("--smooth-radius", "3"), ("--smooth-sigma", "1.5"), ("--smooth-fill", "0")):
        usage_error(infer.main, base + [flag, v], capsys, f"{flag} needs --smooth-tracks")
        usage_error(d_infer.main, base + ["--intrinsics", "K", flag, v], capsys, f"{flag} needs --smooth-tracks")
    usage_error(infer.main, base + ["--smooth-tracks", "--smooth-radius", "33"], capsys, "--smooth-radius must be in 0..32")
    usage_error(infer.main, base + ["--smooth-tracks", "--smooth-sigma", "0"], capsys, "--smooth-sigma must be > 0")
    usage_error(infer.main, base + ["--smooth-tracks", "--smooth-fill", "-1"], capsys, "--smooth-fill must be >= 0")
    a = infer._parser().parse_args(base)
    assert a.smooth_tracks is False and a.smooth_radius is None and a.smooth_sigma is None and a.smooth_fill is None
    a = infer._parser().parse_args(base + ["--smooth-tracks", "--smooth-fill", "0"])
    infer.smooth_args(infer._parser(), a)
    assert (a.smooth_radius, a.smooth_sigma, a.smooth_fill) == (4, 2.0, 0)


def test_evaluate_motion_flags_give_usage_errors(capsys):
    from hamer_yolo_amd import evaluate_motion as EM
    for flag, v in (("--radius", "3"), ("--sigma", "1.5"), ("--max-fill", "1")):
        usage_error(EM.main, ["--pred", "A", flag, v], capsys, f"{flag} needs --smooth-to DIR")
    usage_error(EM.main, ["--pred", "A", "--smooth-to", "B", "--radius", "-1"], capsys, "--radius must be in 0..32")
    usage_error(EM.main, ["--pred", "A", "--smooth-to", "B", "--sigma", "-2"], capsys, "--sigma must be > 0")
    usage_error(EM.main, ["--pred", "A", "--smooth-to", "B", "--max-fill", "-1"], capsys, "--max-fill must be >= 0")
    usage_error(EM.main, ["--pred", "A", "--fps", "0"], capsys, "--fps must be > 0")
    usage_error(EM.main, [], capsys, "--pred")
    a = EM._parser().parse_args(["--pred", "A", "--json", "o.json", "--ckpt", "synthetic:0", "--fps", "30"])
    assert a.json == "o.json" and a.ckpt == "synthetic:0" and a.fps == 30.0 and a.smooth_to is None
