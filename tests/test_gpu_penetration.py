"""GPU checks of hm_mesh_penetration (hamer.utils.penetration) and of the driver that stands on it.  The kernel must EQUAL the
numpy rule of tests/penetration_rule.py on every case: codes, nearest faces, counts, sums and the maximum's bits exactly, and the
signed distances as the same float32 bytes."""
import functools
import json
import os
import sys
import time

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import depth_eval_rule as DR  # noqa: E402
import penetration_rule as PR  # noqa: E402
from test_penetration_host import Q, box_mesh, lattice, octahedron, sphere_pair, star  # noqa: E402

from hamer_yolo_amd import render  # noqa: E402
from hamer_yolo_amd.hamer.utils import penetration as PN  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
NO_FACES = np.zeros((0, 3), np.int32)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def gpu_meshes(meshes):
    return [{"frame": m.get("frame", 0), "vertices": dev(np.asarray(m["vertices"], np.float64)), "faces": dev(np.asarray(m["faces"], np.int32))}
            for m in meshes]


def mesh(v, f=NO_FACES, frame=0):
    return {"frame": frame, "vertices": np.asarray(v, np.float64), "faces": np.asarray(f, np.int32)}


def host(r):
    return {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in r.items()}


def same_as_rule(got, q, want):
    rows = slice(int(got["row_start"][q]), int(got["row_start"][q + 1]))
    assert np.array_equal(got["code"][rows], want["code"]), q
    assert got["signed_distance"][rows].tobytes() == want["signed_distance"].tobytes(), q
    assert np.array_equal(got["nearest_face"][rows], want["nearest_face"]), q
    assert got["sums"][q].tolist() == want["sums"].tolist(), (q, got["sums"][q].tolist(), want["sums"].tolist())


def run_and_compare(meshes, pairs, tol=PN.CONTACT_TOL_M):
    got = host(PN.mesh_penetration(gpu_meshes(meshes), pairs, tol))
    assert got["row_start"].tolist() == np.concatenate([[0], np.cumsum([len(meshes[a]["vertices"]) for a, _ in pairs])]).tolist()
    assert len(got["code"]) == got["row_start"][-1] and got["sums"].shape == (len(pairs), 10)
    wants = [PR.query(meshes[a]["vertices"], meshes[b]["vertices"], meshes[b]["faces"], tol) for a, b in pairs]
    for q, want in enumerate(wants):
        same_as_rule(got, q, want)
    return got, wants


@functools.lru_cache(maxsize=None)
def two_ellipsoids():
    """About 170 faces each, overlapping by a finger's width."""
    v, f = DR.ellipsoid((0.04, 0.07, 0.02), n_lat=8, n_lon=12)
    c, s = np.cos(0.5), np.sin(0.5)
    turned = v @ np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    return mesh(v + (-0.02, 0.0, 0.5), f), mesh(turned + (0.03, 0.01, 0.515), f)


@functools.lru_cache(maxsize=None)
def cloud(n=300, seed=2):
    """Points in and around the first ellipsoid."""
    a, _ = two_ellipsoids()
    rng = np.random.default_rng(seed)
    return rng.uniform(a["vertices"].min(0) - 0.004, a["vertices"].max(0) + 0.004, (n, 3))


# ------------------------------------------------------------------ the ownership rule
def test_cube_and_octahedron_lattices():
    cv, cf = box_mesh((0, 0, 0), (4 * Q, 4 * Q, 4 * Q))
    ov, of = octahedron(4 * Q)
    meshes = [mesh(lattice(-2, 6)), mesh(cv, cf), mesh(lattice(-6, 6)), mesh(ov, of), mesh(ov, of[:, [0, 2, 1]])]
    got, wants = run_and_compare(meshes, [(0, 1), (2, 3), (2, 4)], tol=2 * Q)
    X = np.rint(meshes[0]["vertices"] / Q)
    inside, shell = ((X > 0) & (X < 4)).all(1), ((X >= 0) & (X <= 4)).all(1)
    assert np.array_equal((wants[0]["code"] == PR.INSIDE)[inside | ~shell], inside[inside | ~shell]) and got["sums"][0, PR.N_INSIDE] >= 27
    assert np.array_equal(wants[1]["code"], wants[2]["code"]) and got["sums"][1, PR.N_INSIDE] >= 25


# ------------------------------------------------------------------ shapes
def test_two_ellipsoids_both_directions():
    a, b = two_ellipsoids()
    got, wants = run_and_compare([a, b], [(0, 1), (1, 0)])
    for q in (0, 1):
        s = got["sums"][q]
        assert s[PR.STATUS] == PR.OK and s[PR.N_INSIDE] > 3 and s[PR.N_NEAR] > 0 and 0 < s[PR.TESTED] < len(a["vertices"])
        assert 0.002 < PR.max_depth(s) < 0.03
    assert set(np.unique(got["code"]).tolist()) == {PR.FAR, PR.NEAR, PR.INSIDE}


def test_vertex_counts_around_the_chunk_edges():
    """1, 63, 64, 65 and 257 vertices of a: one lane, a wave short of one, a full chunk, one more, and five chunks."""
    a, _ = two_ellipsoids()
    pts = cloud()
    counts = (1, 63, 64, 65, 257)
    meshes = [a] + [mesh(pts[7:7 + k]) for k in counts]
    got, wants = run_and_compare(meshes, [(i + 1, 0) for i in range(len(counts))], tol=0.003)
    assert [int(s[PR.N_INSIDE]) for s in got["sums"]] == [int((w["code"] == PR.INSIDE).sum()) for w in wants]
    assert got["sums"][4, PR.N_INSIDE] > 20 and got["sums"][4, PR.N_NEAR] > 5


@pytest.mark.parametrize("n_lat,n_lon,faces", [(16, 18, 540), (14, 20, 520), (15, 18, 504)])
def test_face_counts_around_the_lds_tile(n_lat, n_lon, faces):
    """More than one tile of 512 faces and not a multiple of it, a few faces past one tile, and just under one."""
    v, f = DR.ellipsoid((0.04, 0.07, 0.02), n_lat=n_lat, n_lon=n_lon)
    assert len(f) == faces
    a, _ = two_ellipsoids()
    b = mesh(v + (-0.02, 0.0, 0.5), f)
    centre = b["vertices"].mean(0)
    under = mesh((b["vertices"][f[-30:]].mean(1) - centre) * 0.97 + centre)        # just under the last thirty faces
    got, _ = run_and_compare([mesh(cloud(150, seed=n_lat)), b, a, under], [(0, 1), (2, 1), (3, 1)], tol=0.003)
    assert got["sums"][0, PR.N_INSIDE] > 20 and got["sums"][2, PR.N_INSIDE] == 30
    assert sorted(got["nearest_face"][-30:].tolist()) == list(range(faces - 30, faces))


def test_a_star_is_not_convex():
    v, f = star(n_lat=8, n_lon=12, scale=0.04)
    rng = np.random.default_rng(9)
    b = mesh(v + (0.0, 0.0, 0.5), f)
    pts = rng.uniform(b["vertices"].min(0), b["vertices"].max(0), (200, 3))
    got, _ = run_and_compare([mesh(pts), b], [(0, 1)], tol=0.002)
    assert 20 < got["sums"][0, PR.N_INSIDE] < 180


# ------------------------------------------------------------------ the early-out, statuses, invalid data
def test_disjoint_queries_among_overlapping_ones():
    a, b = two_ellipsoids()
    away = mesh(b["vertices"] + (0.0, 0.0, 0.3), b["faces"])
    touching = mesh(a["vertices"] + (0.0815, 0.0, 0.0), a["faces"])       # boxes 1.5 mm apart: inside the tolerance, outside without
    meshes = [a, b, away, touching]
    pairs = [(0, 2), (0, 1), (2, 0), (1, 0), (2, 1), (0, 3), (1, 2), (3, 0)]
    got, _ = run_and_compare(meshes, pairs)
    assert got["sums"][:, PR.STATUS].tolist() == [1, 0, 1, 0, 1, 0, 1, 0]
    got, _ = run_and_compare(meshes, pairs, tol=0.001)
    assert got["sums"][:, PR.STATUS].tolist() == [1, 0, 1, 0, 1, 1, 1, 1]


def test_invalid_data_and_too_large():
    a, b = two_ellipsoids()
    va, vb, f = a["vertices"], b["vertices"], b["faces"]
    bad_a = va.copy()
    bad_a[3, 1], bad_a[5, 2], bad_a[70, 0], bad_a[71, 0] = np.nan, np.inf, 16384.0, -1e300
    bad_b = vb.copy()
    bad_b[9], bad_b[40, 2] = np.nan, -np.inf
    wild = f.copy()
    wild[4, 1], wild[6, 2], wild[8, 0] = len(vb), -1, 2 ** 31 - 1
    flat = np.concatenate([f, [[2, 2, 5], [1, 1, 1], [3, 7, 3]]]).astype(np.int32)
    wide_b, wide_a = vb.copy(), va.copy()
    wide_b[1, 0] = wide_b[:, 0].min() + 2.0
    wide_a[2, 2] = wide_a[:, 2].min() + 2.0
    nearly = vb.copy()
    nearly[1, 0] = np.rint(nearly[:, 0].min() * 65536) * Q + 2.0 - Q
    shifted = mesh(np.rint(va * 65536) * Q + (Q, 0.0, 0.0), a["faces"])   # a against itself, one quantum along x
    meshes = [a, b, mesh(bad_a, a["faces"]), mesh(bad_b, f), mesh(vb, wild), mesh(vb, flat), mesh(wide_b, f), mesh(wide_a, a["faces"]),
              mesh(nearly, f), shifted, mesh(np.full((5, 3), np.nan), f[:3]), mesh(np.zeros((0, 3)))]
    pairs = [(2, 1), (0, 3), (0, 4), (0, 5), (0, 6), (7, 1), (6, 0), (0, 8), (9, 0), (0, 9), (0, 10), (10, 0), (11, 0), (0, 11), (2, 3),
             (2, 6)]
    got, wants = run_and_compare(meshes, pairs, tol=0.001)
    st = got["sums"][:, PR.STATUS].tolist()
    assert st == [0, 0, 0, 0, 2, 2, 2, 0, 0, 0, 1, 1, 1, 1, 0, 2]
    assert got["sums"][0, PR.N_INVALID] == 4 and got["sums"][11, PR.N_INVALID] == 5 and got["sums"][15].tolist() == [0, 0, 0, 0, 2, 0, 0, 0, 0, 0]
    base = PR.query(va, vb, f, 0.001)
    assert wants[3]["sums"].tolist() == base["sums"].tolist()             # faces of area 0 change nothing
    assert got["sums"][8, PR.TESTED] == len(va) and 0 < got["sums"][8, PR.N_INSIDE] < len(va)


# ------------------------------------------------------------------ batch independence
def test_a_query_does_not_depend_on_its_batch():
    a, b = two_ellipsoids()
    pts = cloud()
    others = [mesh(pts[:77]), mesh(pts[100:101]), mesh(b["vertices"] + (0.0, 0.0, 0.3), b["faces"]), mesh(pts[40:300])]
    alone = host(PN.mesh_penetration(gpu_meshes([a, b]), [(0, 1)]))
    want = PR.query(a["vertices"], b["vertices"], b["faces"])
    same_as_rule(alone, 0, want)
    n = len(a["vertices"])
    for place in (0, 3, 7):
        meshes = others + [a, b]
        seven = [(0, 5), (1, 5), (2, 4), (3, 5), (5, 4), (4, 2), (3, 4)]
        pairs = seven[:place] + [(4, 5)] + seven[place:]
        got = host(PN.mesh_penetration(gpu_meshes(meshes), pairs))
        r0 = int(got["row_start"][place])
        for k in ("code", "signed_distance", "nearest_face"):
            assert got[k][r0:r0 + n].tobytes() == alone[k].tobytes(), (place, k)
        assert got["sums"][place].tobytes() == alone["sums"][0].tobytes()
        if place == 3:                                                     # and the seven others equal the rule as well
            for q, (i, j) in enumerate(pairs):
                same_as_rule(got, q, PR.query(meshes[i]["vertices"], meshes[j]["vertices"], meshes[j]["faces"]))
    # many queries: more than one block of the query table (192 per launch), every one the same bytes
    many = host(PN.mesh_penetration(gpu_meshes([a, b]), [(0, 1), (1, 0)] * 100))
    back = PR.query(b["vertices"], a["vertices"], a["faces"])
    for q in (0, 1, 191, 192, 193, 198, 199):
        same_as_rule(many, q, want if q % 2 == 0 else back)
    assert (many["sums"][0::2] == many["sums"][0]).all() and (many["sums"][1::2] == many["sums"][1]).all()


def test_hand_penetration_submits_both_directions():
    a, b = two_ellipsoids()
    lone = mesh(cloud()[:50], frame=1)
    c, d = mesh(a["vertices"] + (0, 0, 0.1), a["faces"], frame=2), mesh(b["vertices"] + (0.005, 0, 0.1), b["faces"], frame=2)
    three = [mesh(a["vertices"], a["faces"], frame=3)] * 3
    meshes = [a, lone, c, b, d] + three                                    # frame 0: rows 0 and 3; frame 2: rows 2 and 4
    got = PN.hand_penetration(gpu_meshes(meshes))
    assert got["hands"] == [(0, 3), (2, 4)] and got["pairs"] == [(0, 3), (3, 0), (2, 4), (4, 2)]
    h = host(got)
    for q, (i, j) in enumerate(got["pairs"]):
        same_as_rule(h, q, PR.query(meshes[i]["vertices"], meshes[j]["vertices"], meshes[j]["faces"]))
    s = PN.summary(got["sums"])
    assert (s["inside"] > 0).all() and s["max_depth_m"][0] == PR.max_depth(h["sums"][0]) and (s["mean_depth_m"] <= s["max_depth_m"]).all()
    none = PN.hand_penetration(gpu_meshes([lone]))
    assert none["pairs"] == [] and none["sums"].shape == (0, 10) and none["code"].numel() == 0
    PN.release_workspaces()


# ------------------------------------------------------------------ resolve
def test_resolve_penetration_equals_the_rule_loop_and_does_not_wait():
    va, vb, f = sphere_pair()
    far = vb + (0.3, 0.0, 0.0)
    ea, eb = two_ellipsoids()
    verts, faces = [va, vb, ea["vertices"], eb["vertices"], va + (0.3, 0.0, 0.0), far + (0.0, 0.0, 0.2)], [f, f, ea["faces"], eb["faces"], f, f]
    pairs = [(0, 1), (3, 2), (4, 5)]
    gm = gpu_meshes([mesh(v, ff) for v, ff in zip(verts, faces)])
    got = PN.resolve_penetration(gm, pairs)
    want_shift, want_last = PR.resolve(verts, faces, pairs, rounds=8, gain=PN.GAIN)
    shift = got["shift"].cpu().numpy()
    print("resolve: largest difference to the rule's loop %.3g m" % np.abs(shift - want_shift).max(), shift[1] - shift[0], shift[3] - shift[2])
    assert np.abs(shift - want_shift).max() <= 1e-9
    assert got["resolved"].tolist() == [True, True, True] and got["pairs"] == [(0, 1), (1, 0), (3, 2), (2, 3), (4, 5), (5, 4)]
    sums = got["sums"].cpu().numpy()
    assert (sums[:, PR.N_INSIDE] == 0).all() and np.array_equal(sums.reshape(3, 2, 10), want_last)
    assert not shift[4:].any() and shift[:4].any(1).all() and np.array_equal(got["shift_quanta"].cpu().numpy() * Q, shift)
    assert abs((shift[1] - shift[0])[2] - 0.03) < 0.004 and np.abs((shift[1] - shift[0])[:2]).max() < 1e-4
    zero = PN.resolve_penetration(gm, pairs, rounds=0)
    assert not zero["shift"].any() and zero["resolved"].tolist() == [False, False, True]
    # half a second of earlier work on the stream is still running when resolve_penetration returns
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    torch.cuda._sleep(1000000)
    t1.record()
    torch.cuda.synchronize()
    spin = int(1000000 * 500.0 / max(t0.elapsed_time(t1), 1e-3))
    torch.cuda._sleep(spin)
    busy = torch.cuda.Event()
    busy.record()
    start = time.perf_counter()
    again = PN.resolve_penetration(gm, pairs)
    waited = busy.query()
    print("resolve_penetration enqueued in %.1f ms" % ((time.perf_counter() - start) * 1e3))
    assert not waited
    assert torch.equal(again["shift_quanta"], got["shift_quanta"]) and torch.equal(again["sums"], got["sums"])
    PN.release_workspaces()


# ------------------------------------------------------------------ the driver, on constructed meshes in place of MANO
class _Mano:
    def __init__(self, faces):
        self.faces = faces


class StubHamer:
    """What the driver reads of a model: the device and the MANO faces -- here an ellipsoid with the cap around one pole cut
    off, open as the MANO wrist is."""
    device = DEV

    def __init__(self):
        v, f = DR.ellipsoid((0.04, 0.07, 0.02), n_lat=8, n_lon=12)
        self.verts = v.astype(np.float32)
        self.mano = _Mano(f[~(f == 0).any(1)])


def _record(cam_ts):
    return {t: None if c is None else {"betas": np.zeros(10, np.float32), "cam_t": np.array(c, np.float32), "is_right": t == "right"}
            for t, c in zip(("right", "left"), cam_ts)}


def test_drivers_on_three_tiny_records(tmp_path, monkeypatch):
    from hamer_yolo_amd import evaluate_penetration as EP
    from hamer_yolo_amd import infer
    hi = StubHamer()
    monkeypatch.setattr(infer, "hamer_inference", lambda cfg: hi)
    monkeypatch.setattr(render, "camera_vertices", lambda hamer, hands: torch.stack(
        [torch.from_numpy(hamer.verts + np.asarray(h["cam_t"], np.float32).reshape(1, 3)) for h in hands]).to(DEV))
    src, out, res_dir = tmp_path / "npy", tmp_path / "out", tmp_path / "resolved"
    src.mkdir()
    place = {"p0": ((0.0, 0.0, 0.5), (0.03, 0.01, 0.51)), "p1": ((-0.1, 0.0, 0.5), (0.1, 0.0, 0.5)), "p2": ((0.0, 0.0, 0.6), None)}
    for stem, cams in place.items():
        np.save(src / f"{stem}.npy", _record(cams))
    res = EP.main(["--pred", str(src), "--contact-tol-mm", "1.5", "--write-to", str(out), "--resolve-to", str(res_dir), "--json",
                   str(tmp_path / "out.json")])
    assert [(r["stem"], r["hand"]) for r in res["rows"]] == [("p0", "right"), ("p0", "left"), ("p1", "right"), ("p1", "left")]
    assert (res["records"], res["two_hand_records"], res["penetrating_records"]) == (3, 2, 1) and PN._ws == {}
    assert res["annotate"] == {"records": 3, "annotated": 2, "penetrating": 1}
    assert res["resolve"] == {"records": 3, "annotated": 2, "moved": 1, "unresolved": 0}
    assert json.load(open(tmp_path / "out.json"))["rows"][1]["inside"] == res["rows"][1]["inside"]
    closed = np.concatenate([hi.mano.faces, PR.close_boundaries(hi.mano.faces, len(hi.verts))])
    assert len(closed) == len(hi.mano.faces) + 10
    for folder in (out, res_dir):
        assert open(folder / "p2.npy", "rb").read() == open(src / "p2.npy", "rb").read()
    for stem in ("p0", "p1"):
        a, b = (np.load(d / f"{stem}.npy", allow_pickle=True).item() for d in (out, src))
        v = [(hi.verts + b[t]["cam_t"].reshape(1, 3)).astype(np.float64) for t in EP.SIDES]
        for k, t in enumerate(EP.SIDES):
            want = PR.query(v[k], v[1 - k], closed, 0.0015)
            h = a[t]
            assert set(h) == set(b[t]) | set(EP.NEW_KEYS) and all(np.array_equal(h[key], b[t][key]) for key in b[t])
            assert h["vertices_contact"].dtype == np.uint8 and np.array_equal(h["vertices_contact"], want["code"])
            assert h["vertices_signed_distance"].tobytes() == want["signed_distance"].tobytes()
            assert h["penetration_depth_m"] == PR.max_depth(want["sums"]) and h["penetration_vertices"] == want["sums"][PR.N_INSIDE]
            assert h["contact_vertices"] == want["sums"][PR.N_NEAR] and (h["penetration_vertices"] > 0) == (stem == "p0")
            assert (h["penetration_mean_m"] > 0) == (stem == "p0") and h["penetration_mean_m"] <= h["penetration_depth_m"]
    # resolved: p0 moved apart and clean by the rule measured from the written cam_t; p1 untouched but for the keys
    for stem in ("p0", "p1"):
        a, b = (np.load(d / f"{stem}.npy", allow_pickle=True).item() for d in (res_dir, src))
        v = [(hi.verts + a[t]["cam_t"].reshape(1, 3)).astype(np.float64) for t in EP.SIDES]
        for k, t in enumerate(EP.SIDES):
            h = a[t]
            assert set(h) == set(b[t]) | set(EP.NEW_KEYS) | set(EP.RESOLVE_KEYS) and h["penetration_resolved"] is True
            assert np.array_equal(h["cam_t_unresolved"], b[t]["cam_t"]) and h["cam_t"].dtype == np.float32
            assert np.array_equal(h["cam_t"], (b[t]["cam_t"].astype(np.float64) + h["penetration_shift_m"].astype(np.float64)).astype(np.float32)) or \
                np.abs(h["cam_t"] - b[t]["cam_t"] - h["penetration_shift_m"]).max() < 1e-7
            assert h["penetration_shift_m"].any() == (stem == "p0") and h["penetration_vertices"] == 0 and h["penetration_depth_m"] == 0.0
            assert PR.query(v[k], v[1 - k], closed, 0.0015)["sums"][PR.N_INSIDE] == 0
    moved = np.load(res_dir / "p0.npy", allow_pickle=True).item()
    assert np.allclose(moved["right"]["penetration_shift_m"], -moved["left"]["penetration_shift_m"], atol=2 * Q)
    # in place, as the infer flags do it
    EP.annotate_folder(str(src), str(src), hi, contact_tol_m=0.0015)
    assert open(src / "p0.npy", "rb").read() == open(out / "p0.npy", "rb").read()
    assert open(src / "p2.npy", "rb").read() == open(out / "p2.npy", "rb").read()
