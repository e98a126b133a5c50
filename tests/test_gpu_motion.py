"""hm_track_smooth and hm_track_jitter (csrc/motion.hip) against tests/motion_rule.py: the kernels must EQUAL the rule, byte for
byte, on every case; then the drivers end to end on a synthetic MANO model."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import motion_rule as MR  # noqa: E402
from test_motion_host import constant_velocity, random_rotations, rotmat  # noqa: E402

from hamer_yolo_amd import lib as L  # noqa: E402
from hamer_yolo_amd.hamer.utils import motion as MO  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
TILE = 32                                   # csrc/motion.hip: frames per workgroup
KEYS = ("rot", "lin", "status", "pairs", "nearest_pair", "moved")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def tracks(N, S, J, C, seed, spread=50.0, share=0.8):
    """Seeded rotations scattered ``spread`` degrees about one rotation per (track, joint), channels, and presence."""
    rng = np.random.default_rng(seed)
    rot = np.moveaxis(random_rotations(rng, (S, J, N), spread), 2, 0) if N * S * J else np.zeros((N, S, J, 3, 3))
    return np.ascontiguousarray(rot), rng.normal(size=(N, S, C)), (rng.uniform(size=(N, S)) < share).astype(np.uint8)


def run(rot, lin, present, radius, sigma=2.0):
    got = MO.track_smooth(dev(rot), dev(lin), dev(present), radius, sigma)
    return {k: got[k].cpu().numpy() for k in KEYS}


def same(got, want, where=None, what=""):
    pick = (lambda a: a) if where is None else (lambda a: a[where])
    for k in ("status", "pairs", "nearest_pair"):
        assert got[k].dtype == np.int32 and np.array_equal(pick(got[k]), pick(want[k])), (what, k)
    for k in ("rot", "lin", "moved"):
        a, b = np.ascontiguousarray(pick(got[k])), np.ascontiguousarray(pick(want[k]))
        assert a.dtype == np.float64 and a.shape == b.shape, (what, k)
        if a.tobytes() != b.tobytes():
            bad = np.argwhere(a.view(np.uint64) != b.view(np.uint64))
            raise AssertionError(f"{what}: {k} differs from the rule at {len(bad)} of {a.size} elements, first {bad[0].tolist()}: "
                                 f"{a[tuple(bad[0])]!r} != {b[tuple(bad[0])]!r}")


def equals_rule(rot, lin, present, radius, sigma=2.0, what=""):
    got = run(rot, lin, present, radius, sigma)
    want = MR.track_smooth(rot, lin, present, MR.window_weights(radius, sigma))
    same(got, want, what=what)
    return got


# ------------------------------------------------------------------ hm_track_smooth
@pytest.mark.parametrize("R", [0, 1, 5, 32])
def test_frame_counts_around_the_tile(R):
    seen = set()
    for N in (1, 2, 3, TILE - 1, TILE, TILE + 1, TILE + R, 2 * TILE + 1):
        rot, lin, present = tracks(N, 2, 16, 13, seed=100 * R + N)
        got = equals_rule(rot, lin, present, R, what=f"N={N} R={R}")
        seen |= set(got["status"].reshape(-1).tolist())
        if R == 0:
            assert not got["pairs"].any()
    assert seen >= ({MR.KEPT, MR.ABSENT} if R == 0 else {MR.KEPT, MR.SMOOTHED, MR.FILLED, MR.ABSENT})


@pytest.mark.parametrize("R", [1, 5])
def test_presence_patterns(R):
    N = 2 * TILE + 7
    rot, lin, _ = tracks(N, 2, 16, 13, seed=7 + R, spread=30.0)
    t = np.arange(N)
    single = (t == TILE).astype(np.uint8)
    run_r, run_r1 = np.ones(N, np.uint8), np.ones(N, np.uint8)
    run_r[10:10 + R] = 0; run_r[TILE - 2:TILE - 2 + R] = 0               # absent runs of exactly R, one across the tile edge
    run_r1[10:11 + R] = 0; run_r1[TILE - 2:TILE - 1 + R] = 0             # and of R + 1
    patterns = {"all": (np.ones(N, np.uint8),) * 2, "none": (np.zeros(N, np.uint8),) * 2,
                "alternating": ((t % 2).astype(np.uint8), ((t + 1) % 2).astype(np.uint8)), "single": (single, np.roll(single, 5)),
                "runs": (run_r, run_r1), "different": (np.ones(N, np.uint8), (t % 3 != 0).astype(np.uint8))}
    for name, (a, b) in patterns.items():
        got = equals_rule(rot, lin, np.stack([a, b], 1), R, what=f"{name} R={R}")
        if name == "none":
            assert (got["status"] == MR.ABSENT).all() and np.isnan(got["rot"]).all() and np.isnan(got["lin"]).all()
        if name == "runs":                                                # a run of R is bridged everywhere, a run of R + 1 is not
            assert (got["status"][10:10 + R, 0] == MR.FILLED).all() and (got["status"][10:11 + R, 1] == MR.ABSENT).any()
        if name == "single":
            assert sorted(np.unique(got["status"]).tolist()) == [MR.KEPT, MR.ABSENT]


@pytest.mark.parametrize("S", [1, 2, 5])
def test_shapes(S):
    for J in (1, 16, 17):
        for C in (0, 1, 13):
            rot, lin, present = tracks(TILE + 3, S, J, C, seed=S * 1000 + J * 10 + C)
            equals_rule(rot, lin, present, 3, what=f"S={S} J={J} C={C}")


def test_one_degenerate_joint_keeps_the_whole_hand():
    N, R = 9, 2
    rot, lin, _ = tracks(N, 2, 16, 13, seed=21, spread=10.0)
    present = np.ones((N, 2), np.uint8)
    # joint 9 of track 0 turns by 180 degrees every frame about a fixed axis: every pair sum around frame 4 cancels its centre
    for t in range(N):
        rot[t, 0, 9] = rotmat([0.0, np.pi * (t % 2), 0.0])
    present[4, 1] = 0
    rot[2:4, 1, 12] = rotmat([0.0, 0.0, 0.0]); rot[5:7, 1, 12] = rotmat([np.pi, 0.0, 0.0])  # across the gap of track 1
    w = np.array([1.0, 1.0, 0.5])
    got = MO.track_smooth(dev(rot), dev(lin), dev(present), weights=w)
    got = {k: got[k].cpu().numpy() for k in KEYS}
    same(got, MR.track_smooth(rot, lin, present, w), what="degenerate")
    assert got["status"][4, 0] == MR.DEGENERATE and got["status"][4, 1] == MR.DEGENERATE and got["pairs"][4].tolist() == [2, 2]
    assert got["rot"][4, 0].tobytes() == rot[4, 0].tobytes() and got["lin"][4, 0].tobytes() == lin[4, 0].tobytes()
    assert np.isnan(got["rot"][4, 1]).all() and np.isnan(got["lin"][4, 1]).all() and np.isnan(got["moved"][4]).all()
    assert (got["status"][[0, N - 1]] == MR.KEPT).all() and (got["status"] == MR.SMOOTHED).any()


def test_a_frame_does_not_depend_on_its_batch():
    R, N = 5, TILE + 9
    rot, lin, present = tracks(N + 20, 2, 16, 13, seed=33)
    base = run(rot[:N], lin[:N], present[:N], R)
    # extended beyond the window: frames whose window lay inside the first N keep their bytes
    longer = run(rot, lin, present, R)
    inside = slice(0, N - R)
    same({k: v[:N] for k, v in longer.items()}, base, where=inside, what="extended")
    # a second track added
    one = run(rot[:N, :1], lin[:N, :1], present[:N, :1], R)
    same({k: v[:, :1] for k, v in base.items()}, one, what="second track")
    # shifted by one absent frame in front: the tile boundaries move
    pad = lambda a: np.concatenate([np.zeros_like(a[:1]), a[:N]])        # noqa: E731
    shifted = run(pad(rot), pad(lin), pad(present), R)
    same({k: v[1:] for k, v in shifted.items()}, base, what="shifted")


def test_constant_velocity_comes_back():
    rng = np.random.default_rng(3)
    rot, lin = constant_velocity(60, 2, 16, 13, rng)
    present = (rng.uniform(size=(60, 2)) > 0.25).astype(np.uint8)
    got = equals_rule(rot, lin, present, 6, what="constant velocity")
    ok = got["status"] != MR.ABSENT
    assert (got["status"] == MR.FILLED).sum() >= 5 and np.abs(got["rot"][ok] - rot[ok]).max() < 1e-12


def test_empty_sequences_launch_nothing():
    for N, S in ((0, 2), (3, 0), (0, 0)):
        r = MO.track_smooth(torch.zeros(N, S, 16, 3, 3, dtype=torch.float64, device=DEV), torch.zeros(N, S, 13, dtype=torch.float64, device=DEV),
                            torch.zeros(N, S, dtype=torch.uint8, device=DEV))
        assert tuple(r["rot"].shape) == (N, S, 16, 3, 3) and tuple(r["status"].shape) == (N, S)
        assert tuple(MO.track_jitter(torch.zeros(N, S, 21, 3, dtype=torch.float64, device=DEV), torch.zeros(N, S, dtype=torch.uint8, device=DEV)).shape) == (N, S)


# ------------------------------------------------------------------ hm_track_jitter
@pytest.mark.parametrize("P", [1, 21, 63, 64, 65, 778, 1024])
def test_jitter_equals_the_rule(P):
    rng = np.random.default_rng(P)
    N, S = 11, 3
    x = rng.normal(size=(N, S, P, 3))
    present = np.ones((N, S), np.uint8)
    present[5, 1] = 0; present[0, 2] = 0; present[7:9, 2] = 0
    got = MO.track_jitter(dev(x), dev(present)).cpu().numpy()
    want = MR.track_jitter(x, present)
    assert got.dtype == np.float64 and got.tobytes() == want.tobytes()
    assert np.isnan(got[[0, N - 1]]).all() and np.isnan(got[4:7, 1]).all() and np.isnan(got[[1, 6, 7, 8, 9], 2]).all()
    assert np.isfinite(got[1:N - 1, 0]).all() and np.isfinite(got[[1, 2, 3, 7, 8, 9], 1]).all()


def test_jitter_of_a_parabola_is_its_second_difference():
    rng = np.random.default_rng(1)
    N, S, P = 8, 2, 21
    a = rng.integers(-8, 9, size=(1, S, P, 3)).astype(np.float64) / 8.0   # exact arithmetic: small dyadic coefficients
    b, c = rng.integers(-8, 9, size=(2, 1, S, P, 3)).astype(np.float64)
    t = np.arange(N, dtype=np.float64)[:, None, None, None]
    x = a * t * t + b * t + c
    got = MO.track_jitter(dev(x), dev(np.ones((N, S), np.uint8))).cpu().numpy()
    assert got.tobytes() == MR.track_jitter(x, np.ones((N, S), np.uint8)).tobytes()
    want = np.linalg.norm(2.0 * a, axis=-1).mean(-1)[0]
    assert np.allclose(got[1:-1], want[None], rtol=1e-14, atol=0) and np.isnan(got[[0, -1]]).all()
    # three frames are the smallest sequence with a value
    short = MO.track_jitter(dev(x[:3]), dev(np.ones((3, S), np.uint8))).cpu().numpy()
    assert np.isnan(short[[0, 2]]).all() and short[1].tobytes() == got[1].tobytes()


# ------------------------------------------------------------------ usage errors
def test_usage_errors():
    rot, lin, present = (dev(a) for a in tracks(4, 2, 16, 13, seed=1))
    with pytest.raises(ValueError):
        MO.track_smooth(rot, lin, present, radius=33)
    with pytest.raises(ValueError):
        MO.track_smooth(rot.cpu(), lin, present)
    with pytest.raises(ValueError):
        MO.track_smooth(rot, lin, present.cpu())
    with pytest.raises(ValueError):
        MO.track_jitter(torch.zeros(3, 2, 1025, 3, dtype=torch.float64, device=DEV), present[:3])
    with pytest.raises(ValueError):
        MO.track_jitter(torch.zeros(3, 2, 21, 3, dtype=torch.float64), present[:3])
    # the entry points themselves: status codes through L.check
    import ctypes as C
    lib = L.load()
    w = np.ones(34)
    wp = w.ctypes.data_as(C.POINTER(C.c_double))
    out = MO.track_smooth(rot, lin, present)
    args = lambda R, rp=L.ptr(rot): (rp, L.ptr(lin), L.ptr(present), 4, 2, 16, 13, wp, R, L.ptr(out["rot"]), L.ptr(out["lin"]),  # noqa: E731
                                     L.ptr(out["status"]), L.ptr(out["pairs"]), L.ptr(out["nearest_pair"]), L.ptr(out["moved"]), None)
    for bad in (args(33), args(-1), args(4, None)):
        with pytest.raises(L.HipLibraryError, match="hm_track_smooth"):
            L.check(lib.hm_track_smooth(*bad), "hm_track_smooth")
    acc = torch.zeros(3, 2, dtype=torch.float64, device=DEV)
    pts = torch.zeros(3, 2, 1025, 3, dtype=torch.float64, device=DEV)
    for bad in ((L.ptr(pts), L.ptr(present), 3, 2, 1025, L.ptr(acc), None), (None, L.ptr(present), 3, 2, 21, L.ptr(acc), None)):
        with pytest.raises(L.HipLibraryError, match="hm_track_jitter"):
            L.check(lib.hm_track_jitter(*bad), "hm_track_jitter")
    torch.cuda.synchronize()


# ------------------------------------------------------------------ the drivers, on a synthetic MANO model
class _Cfg:
    ckpt_path = "synthetic:0"
    model_cfg = None
    use_onnx = False
    onnx_path = None


SEED = 5
ABSENT = {("right", 5), ("left", 18), ("left", 24)}                        # two with both neighbours, one at the end
FLIP = ("right", 14)


def synthetic_records():
    """24 records f_1 .. f_24: both hands on a smooth motion plus seeded noise, three hands absent, one global flip."""
    rng = np.random.default_rng(SEED)
    recs = {}
    start = {s: (rng.normal(size=(16, 3)) * 0.25, rng.normal(size=(16, 3)) * 0.02, rng.normal(size=10) * 0.5) for s in ("right", "left")}
    for i in range(1, 25):
        rec = {}
        for s in ("right", "left"):
            a0, rate, betas = start[s]
            aa = a0 + rate * i + 0.1 * np.sin(i / 5.0) + rng.normal(size=(16, 3)) * np.radians(3.0)
            if (s, i) == FLIP:
                aa[0] = (aa[0] / np.linalg.norm(aa[0])) * (np.linalg.norm(aa[0]) + np.radians(150.0))
            cam_t = np.array([0.1 if s == "right" else -0.1, 0.02 * np.sin(i / 4.0), 0.5 + 0.004 * i]) + rng.normal(size=3) * 0.002
            aa = aa.astype(np.float32)
            rec[s] = None if (s, i) in ABSENT else {
                "betas": (betas + rng.normal(size=10) * 0.05).astype(np.float32), "theta": aa.reshape(-1), "pose_hand": aa[1:].reshape(-1),
                "pose_global": aa[0].copy(), "cam_t": cam_t.astype(np.float32), "is_right": s == "right"}
        recs[f"f_{i}"] = rec
    return recs


def test_drivers_on_a_synthetic_sequence(tmp_path):
    from hamer_yolo_amd import evaluate_motion as EM
    from hamer_yolo_amd import infer
    hi = infer.hamer_inference(_Cfg)
    src, out = tmp_path / "npy", tmp_path / "smooth"
    src.mkdir()
    recs = synthetic_records()
    for stem, rec in recs.items():
        np.save(src / f"{stem}.npy", rec)
    before = EM.score_folder(str(src), hi, fps=30.0)
    res = EM.smooth_folder(str(src), str(out), hi, radius=4, sigma=2.0, max_fill=2)
    after = EM.score_folder(str(out), hi, fps=30.0)
    assert before["records"] == 24 and before["hands"] == 45 and after["hands"] == 47
    for name in EM.POINT_SETS:                                            # the acceleration of every point set drops
        b, a = before[name]["all"], after[name]["all"]
        print(f"{name}: mean acceleration {b['mean']:.3f} -> {a['mean']:.3f} mm/frame^2 over {b['n']} -> {a['n']} frames")
        assert a["mean"] < b["mean"] and a["n"] > b["n"] and a["mean_m_s2"] == pytest.approx(a["mean"] * 1e-3 * 900.0)
        assert all(after[name][s]["mean"] < before[name][s]["mean"] for s in ("right", "left"))
    got = {s: r for s, _, r in EM.load_sequence(str(out))}
    assert list(got) == [f"f_{i}" for i in range(1, 25)]                 # not the lexicographic order
    for side, i in ABSENT:
        h = got[f"f_{i}"][side]
        if i == 24:
            assert h is None                                              # an end has no pair
        else:
            assert h["track_filled"] is True and h["track_status"] == "FILLED" and h["is_right"] == (side == "right")
            near = [got[f"f_{j}"][side]["cam_t"] for j in (i - 1, i + 1)]
            assert np.abs(h["cam_t"] - (near[0] + near[1]) / 2).max() < 0.01
    assert res["filled"] == 2 and res["degenerate"] == 0 and res["smoothed"] + res["kept"] == 45 and res["kept"] >= 4
    assert res["max_moved_stem"] == f"f_{FLIP[1]}" and 100.0 < res["max_moved_deg"] < 150.0
    flipped = got[f"f_{FLIP[1]}"][FLIP[0]]
    assert int(np.argmax(flipped["track_moved_deg"])) == 0 and flipped["track_status"] == "SMOOTHED"
    assert np.array_equal(flipped["pose_global_unsmoothed"], recs[f"f_{FLIP[1]}"][FLIP[0]]["pose_global"])
    first = got["f_1"]["right"]
    assert first["track_status"] == "KEPT" and all(np.array_equal(first[k], recs["f_1"]["right"][k]) for k in recs["f_1"]["right"])
    # in place: the same bytes as into a second folder
    EM.smooth_folder(str(src), str(src), hi, radius=4, sigma=2.0, max_fill=2)
    for i in range(1, 25):
        assert open(src / f"f_{i}.npy", "rb").read() == open(out / f"f_{i}.npy", "rb").read()


def test_infer_smooth_tracks_rewrites_in_place_and_is_off_by_default(tmp_path, monkeypatch):
    from PIL import Image
    from hamer_yolo_amd import evaluate_motion as EM
    from hamer_yolo_amd import infer, render, synth
    hi = infer.hamer_inference(_Cfg, precise=True)
    rgb, masks = tmp_path / "rgb", tmp_path / "masks"
    rgb.mkdir(); masks.mkdir()
    for k, i in enumerate((1, 2, 10)):
        Image.fromarray(synth.frame_u8(240, 320, seed=70 + k).numpy()[:, :, ::-1]).save(rgb / f"g_{i}.png")
        m = np.zeros((240, 320), np.uint8)
        m[60 + 10 * k:150, 90:170 + 10 * k] = 3
        np.save(masks / f"g_{i}.npy", m)
    monkeypatch.setattr(infer, "hamer_inference", lambda cfg: hi)
    outs = [str(tmp_path / d) for d in ("plain", "flag", "call")]
    infer.main(["--input", str(rgb), "--output", outs[0], "--masks", str(masks)])
    infer.main(["--input", str(rgb), "--output", outs[1], "--masks", str(masks), "--smooth-tracks", "--smooth-radius", "1"])
    r = EM.smooth_folder(outs[0], outs[2], hi, radius=1, sigma=2.0, max_fill=2)
    assert r["records"] == 3 and r["smoothed"] == 1 and r["kept"] == 2
    for f in ("g_1.npy", "g_2.npy", "g_10.npy"):
        raw = [open(os.path.join(o, f), "rb").read() for o in outs]
        assert raw[1] == raw[2] != raw[0]
    mid = np.load(os.path.join(outs[1], "g_2.npy"), allow_pickle=True).item()["right"]
    assert mid["track_status"] == "SMOOTHED" and mid["track_pairs"] == 1
    render.release_workspaces()
