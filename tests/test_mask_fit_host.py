"""Host checks of the mask fit (hm_mask_fit, hamer.utils.mask_eval.mask_fit / fit_contour, evaluate_masks --refine-to, infer
--mask-fit): the numpy rule of tests/mask_fit_rule.py against a brute-force match over all pairs and against normal equations
built term by term in Python integers and fractions; its solve against numpy.linalg.solve; identical and degenerate images; the
contour loop on renders of tests/zrender_rule.py; the folding of a fit into a record; and the surface -- exports, header, build
list, argument checks, the drivers' parsers.  No GPU.

Bounds.  Matches, sums and counts are integers: exact equality.  The solve is compared with numpy.linalg.solve of the same M
within BOUND_C * cond(M) * 2^-53 * max|x|: tests/test_gpu_depth_fit.py takes 64 for its 6 x 6 Cholesky solve, and the constant of
that backward-error bound grows as n (3 n + 1) (114 for n = 6, 52 for n = 4), so BOUND_C = 64 * 52 / 114 = 29.2; cond(M) <=
COND_MAX is asserted on the inputs."""
import ctypes as C
import inspect
import os
import re
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import depth_eval_rule as DR  # noqa: E402
import mask_eval_rule as ER  # noqa: E402
import mask_fit_rule as MR  # noqa: E402
import zrender_rule as ZR  # noqa: E402

from hamer_yolo_amd import build as B  # noqa: E402
from hamer_yolo_amd import lib as L  # noqa: E402
from hamer_yolo_amd.hamer.utils import mask_eval as ME  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND_C = 64.0 * (4 * 13) / (6 * 19)
COND_MAX = 1e5
HOST_END_J = 0.9902         # what the rule's loop reaches on the ellipsoid case on the CPU: J 0.99016 measured
HOST_END_MM = 1.61          # and its mean vertex error: 1.602 mm measured (24.6 mm at the start, 20 mm of it the 4 % in depth)


def brute_nearest(a, b, r):
    """Every set pixel of a against ALL set pixels of b: the least (d2, dy, dx) with d2 <= r r, or None."""
    out = {}
    bs = [(int(y), int(x)) for y, x in zip(*np.nonzero(b))]
    for y, x in zip(*np.nonzero(a)):
        best = None
        for by, bx in bs:
            dx, dy = bx - int(x), by - int(y)
            key = (dx * dx + dy * dy, dy, dx)
            if key[0] <= r * r and (best is None or key < best):
                best = key
        out[(int(y), int(x))] = best
    return out


# ------------------------------------------------------------------ matching
@pytest.mark.parametrize("seed,H,W,r", [(1, 23, 31, 3), (2, 19, 70, 5), (3, 30, 41, 64), (4, 17, 29, 0), (5, 25, 33, 1), (6, 40, 70, 9)])
def test_matching_against_brute_force(seed, H, W, r):
    a, b = ER.bmap(ER.blobs(H, W, seed)), ER.bmap(ER.blobs(H, W, seed + 100))
    assert a.sum() > 20 and b.sum() > 20
    for A, Bm in ((a, b), (b, a)):
        ys, xs, dx, dy, found = MR.nearest(A, Bm, r)
        want = brute_nearest(A, Bm, r)
        assert len(ys) == len(want) == A.sum()
        for k in range(len(ys)):
            w = want[(int(ys[k]), int(xs[k]))]
            assert (w is None) == (not found[k])
            if w is not None:
                assert (int(dx[k]), int(dy[k])) == (w[2], w[1]), (ys[k], xs[k], dx[k], dy[k], w)
        if r >= 3:
            assert found.any()
        if r <= 1:
            assert not found.all()


def test_tie_shapes():
    """A pred boundary pixel midway between two gt boundary pixels in x, in y and diagonally: the least dy wins, then the
    least dx -- and the brute-force search agrees on every pixel."""
    (px, gx), (py, gy), (pd, gd) = MR.tie_shapes()
    for pred, gt, at, want in ((px, gx, (4, 5), (-3, 0)), (py, gy, (4, 5), (0, -3)), (pd, gd, (4, 5), (-3, -3))):
        a, b = ER.bmap(pred), ER.bmap(gt)
        assert a[at] and b[at[0] + want[1], at[1] + want[0]] and b[at[0] - want[1], at[1] - want[0]]     # both candidates exist
        ys, xs, dx, dy, found = MR.nearest(a, b, 6)
        k = int(np.nonzero((ys == at[0]) & (xs == at[1]))[0][0])
        assert found[k] and (int(dx[k]), int(dy[k])) == want
        brute = brute_nearest(a, b, 6)
        for k in range(len(ys)):
            w = brute[(int(ys[k]), int(xs[k]))]
            assert found[k] and (int(dx[k]), int(dy[k])) == (w[2], w[1])
        ys, xs, dx, dy, found = MR.nearest(b, a, 6)                                     # and the other way round
        brute = brute_nearest(b, a, 6)
        assert all((int(dx[k]), int(dy[k])) == brute[(int(ys[k]), int(xs[k]))][2:0:-1] for k in range(len(ys)) if found[k])


# ------------------------------------------------------------------ sums
def explicit(pred, gt, centre, r, reach, directions):
    """The normal equations term by term from explicit per-pixel rows: Python integers, and one Fraction per divided term,
    rounded ONCE to a double (float(Fraction) is correctly rounded, as an IEEE division is).  Returns (sums, counts, rows):
    rows = (weighted 4-vectors as Fractions, right-hand sides) for an independent float build."""
    sums, counts = [0] * 18, [[0] * 6 for _ in range(2)]
    rows = []
    bp, bg = ER.bmap(pred), ER.bmap(gt)
    for k, (A, Bm) in enumerate(((bp, bg), (bg, bp))):
        if not (directions >> k) & 1:
            continue
        for (y, x), m in brute_nearest(A, Bm, r).items():
            counts[k][0] += 1
            if m is None:
                counts[k][3] += 1
                continue
            d2, dy, dx = m
            if k == 0:
                ux, uy, ex, ey = x - centre[0], y - centre[1], dx, dy
            else:
                ux, uy, ex, ey = x + dx - centre[0], y + dy - centre[1], -dx, -dy
            if ux * ux + uy * uy > reach * reach:
                counts[k][4] += 1
                continue
            if d2 == 0:
                counts[k][2] += 1
                sums[15] += ux; sums[16] += uy; sums[17] += ux * ux + uy * uy
                rows.append(((ux, -uy, 1, 0), 0, 1)); rows.append(((uy, ux, 0, 1), 0, 1))
                continue
            counts[k][1] += 1
            J = (ex * ux + ey * uy, ey * ux - ex * uy, ex, ey)
            n = 0
            for i in range(4):
                for j in range(i, 4):
                    sums[n] += int(np.rint(float(Fraction(J[i] * J[j], d2)) * 2.0 ** 20))
                    n += 1
            for i in range(4):
                sums[10 + i] += J[i]
            sums[14] += d2
            rows.append((J, d2, d2))                                                    # row, residual, 1 / weight
    return sums, counts, rows


@pytest.mark.parametrize("seed,H,W,r,reach,directions,centre", [
    (11, 23, 31, 4, 4096, 3, (15, 11)), (12, 19, 70, 6, 20, 1, (30, 9)), (13, 30, 41, 64, 4096, 2, (-7, 50)),
    (14, 25, 33, 2, 9, 3, (16, 12)), (15, 40, 70, 9, 4096, 3, (100000, -3))])
def test_sums_term_by_term(seed, H, W, r, reach, directions, centre):
    pred, gt = ER.blobs(H, W, seed), ER.blobs(H, W, seed + 100)
    gt |= np.roll(pred, 1, axis=1) & (np.arange(W) % 7 < 3)[None, :]                     # so that some contours coincide: anchors
    sums, counts = MR.fit_pair(pred, gt, centre, r, reach, directions)
    want_s, want_c, rows = explicit(pred, gt, centre, r, reach, directions)
    assert counts.tolist() == want_c and [int(v) for v in sums] == want_s
    assert (counts[:, 0] == counts[:, 1:5].sum(1)).all() and (counts[:, 5] == 0).all()
    for k in (0, 1):
        if not (directions >> k) & 1:
            assert (counts[k] == 0).all()
    if centre[0] > 50000:
        assert counts[:, 1].sum() + counts[:, 2].sum() == 0 and counts[:, 4].sum() > 0 and (sums == 0).all()
        return
    assert counts[:, 1].sum() > 20
    if seed in (11, 15):
        assert counts[:, 2].sum() > 0
    if reach < 100:
        assert counts[:, 4].sum() > 0
    # M and g of the rule are the normal equations of the rows: sum of row^T row / weight, within the 2^-21 a term is rounded by
    M, g = MR.matrix(sums, counts, 0.0, 1.0)
    A, b = np.zeros((4, 4)), np.zeros(4)
    for J, rho, w in rows:
        J = np.array(J, np.float64)
        A += np.outer(J, J) / w
        b += J * rho / w
    bound = len(rows) * 2.0 ** -21 + 1e-12 * np.abs(A).max()
    assert np.abs(M - A).max() <= bound and np.abs(g - b).max() <= 1e-9 * max(1.0, np.abs(b).max())


def test_term_bound():
    """|Jr_i Jr_j| / d2 <= max(|u|^2, 1): Cauchy-Schwarz on d.u and d.Ju, and |d_i d_j| <= d2.  With |u|^2 <= reach^2 <= 2^24 a
    term is at most 2^44 < 2^45, so 2^18 pixels stay below 2^63."""
    rng = np.random.default_rng(3)
    d = rng.integers(-64, 65, (20000, 2))
    d = d[(d * d).sum(1) > 0]
    u = rng.integers(-2896, 2897, (len(d), 2))
    J = np.stack([d[:, 0] * u[:, 0] + d[:, 1] * u[:, 1], d[:, 1] * u[:, 0] - d[:, 0] * u[:, 1], d[:, 0], d[:, 1]], 1)
    t = MR.terms(J, (d * d).sum(1))
    assert (np.abs(t[:, :10]) <= np.maximum((u * u).sum(1), 1)[:, None] * 2 ** 20).all() and 4096 * 4096 * 2 ** 20 * 2 ** 18 < 2 ** 63


# ------------------------------------------------------------------ solve
def test_solve_against_numpy():
    seen = 0
    for seed, r, damping, lever in ((21, 5, 1e-3, 50.0), (22, 9, 0.0, 50.0), (23, 3, 1e-2, 10.0), (24, 12, 1e-3, 20.0)):
        pred, gt = ER.blobs(40, 70, seed), None
        gt = np.roll(np.roll(pred, 2, axis=1), -1, axis=0)                             # the same blobs two pixels east, one north
        sums, counts = MR.fit_pair(pred, gt, (35, 20), r, 4096, 3)
        used = MR.used_of(counts)
        assert used >= 50
        M, g = MR.matrix(sums, counts, damping, lever)
        cond = np.linalg.cond(M)
        assert cond <= COND_MAX, cond
        sol = MR.solve(sums[None], counts[None], damping, lever, 30)[0]
        want = np.linalg.solve(M, g)
        bound = BOUND_C * cond * 2.0 ** -53 * np.abs(want).max()
        assert sol[5] == 1.0 and (np.abs(sol[:4] - want) <= bound).all(), (sol[:4], want, bound)
        assert sol[4] == np.sqrt(np.float64(int(sums[14])) / np.float64(used)) and sol[6] == sol[7] == 0.0
        assert 0.0 < sol[2] < 2.5 and abs(sol[0]) < 0.05 and abs(sol[1]) < 0.05          # a step towards the shift, no scale, no turn
        assert MR.solve(sums[None], counts[None], damping, lever, used + 1)[0].tolist() == [0.0] * 4 + [sol[4]] + [0.0] * 3
        seen += 1
    assert seen == 4
    rng = np.random.default_rng(0)
    A = rng.normal(size=(4, 4))
    M, g = A @ A.T + 0.1 * np.eye(4), rng.normal(size=4)
    x, ok = MR.cholesky_solve(M, g)
    assert ok and np.allclose(x, np.linalg.solve(M, g), rtol=1e-10)
    M[2, :], M[:, 2] = 0.0, 0.0
    assert not MR.cholesky_solve(M, g)[1]


def test_identical_images_are_all_anchors():
    for seed in (31, 32):
        s = ER.blobs(40, 70, seed)
        for directions in (1, 2, 3):
            sums, counts = MR.fit_pair(s, s, (33, 17), 5, 4096, directions)
            nb = int(ER.bmap(s).sum())
            for k in (0, 1):
                assert counts[k].tolist() == ([nb, 0, nb, 0, 0, 0] if (directions >> k) & 1 else [0] * 6)
            assert (sums[:15] == 0).all() and sums[17] > 0
            sol = MR.solve(sums[None], counts[None], 1e-3, 50.0, 30)[0]
            assert sol.tobytes() == np.array([0, 0, 0, 0, 0, 1.0, 0, 0], np.float64).tobytes()       # exactly 0, and solved


def test_degenerate_images_are_not_solved():
    H, W = 12, 70
    blob = ER.blobs(H, W, 41)
    for pred, gt in ((np.zeros((H, W), bool), blob), (np.ones((H, W), bool), blob), (blob, np.zeros((H, W), bool)),
                     (blob, np.ones((H, W), bool)), (np.zeros((H, W), bool), np.ones((H, W), bool))):
        sums, counts = MR.fit_pair(pred, gt, (30, 6), 64, 4096, 3)
        assert counts[:, 1].sum() == counts[:, 2].sum() == 0 and (sums == 0).all()
        assert counts[:, 0].sum() == counts[:, 3].sum()                                # what boundary there is, is unmatched
        sol = MR.solve(sums[None], counts[None], 1e-3, 50.0, 1)[0]
        assert sol.tobytes() == np.zeros(8).tobytes()                                  # no NaN: zeros, the flag 0
    # a frame outside the batch is not read
    pid, mask = np.zeros((1, H, W), np.int32), np.zeros((1, H, W), np.uint8)
    sums, counts = MR.fit(pid, mask, [(1, 0, 1, 3), (-1, 0, 1, 3)], np.zeros((2, 2), np.int64), 5, 4096, 3)
    assert (sums == 0).all() and (counts == 0).all()


# ------------------------------------------------------------------ the contour loop on the rule's renders
SCENE = dict(H=240, W=320, K=np.array([[600.0, 0, 160.0], [0, 600.0, 120.0], [0, 0, 1.0]]), centre=np.array([0.03, -0.02, 0.5]),
             semi=(0.04, 0.09, 0.02), shift=(0.010, -0.008), depth=1.04, degrees=8.0, radius=16, label=3)


def ellipsoid_scene():
    """The depth tests' ellipsoid scene, the ellipsoid scaled so that its silhouette is clearly not a circle: semi-axes 40 and
    90 mm across the viewing axis (48 x 108 pixels at 0.5 m) instead of 50 and 80.  The mask is the true pose's silhouette; the
    start is (10, -8) mm off in the image plane, 4 % too far and turned by 8 degrees about the viewing axis."""
    v, f = DR.ellipsoid(semi=SCENE["semi"])
    c = SCENE["centre"]
    Rz = MR.exp_so3(np.array([[0.0, 0.0, np.radians(SCENE["degrees"])]]))[0]
    verts = (v @ Rz.T)[None].astype(np.float32)
    start = ((c + np.array([*SCENE["shift"], 0.0])) * np.array([1.0, 1.0, SCENE["depth"]]))[None].astype(np.float32)
    return v, f, (v + c)[None], verts, start


def jaccard(mid, mask):
    return ER.jf(ER.counts(mid >= 0, mask == SCENE["label"], 4))[0]


def test_contour_loop_on_the_ellipsoid():
    v, f, truth, verts, start = ellipsoid_scene()
    H, W, K = SCENE["H"], SCENE["W"], SCENE["K"]

    def render(placed):
        meshes = [{"frame": j, "vertices": placed[j], "faces": f, "face_id0": j * len(f)} for j in range(len(placed))]
        return ZR.render(len(placed), H, W, K, meshes)["mesh_id"]

    mask = (render(truth.astype(np.float32)) >= 0).astype(np.uint8) * SCENE["label"]
    cams = np.array([[600.0, 600.0, 160.0, 120.0]])
    r = MR.fit_contour(render, verts, start, start.astype(np.float64), [0], mask, [SCENE["label"]], cams, rounds=6, radius=SCENE["radius"])
    Js = [jaccard(render(p)[0], mask[0]) for p in r["trail"]]
    errs = [float(np.linalg.norm(p - truth, axis=2).mean() * 1e3) for p in r["trail"]]
    print("J per round", ["%.5f" % j for j in Js], "mean vertex error in mm", ["%.3f" % e for e in errs],
          "rms %.3f px over %d pixels" % (r["rms"][0], r["pixels"][0]))
    assert Js[0] < 0.8 and errs[0] > 20.0                                              # the start is well off
    assert all(b >= a - 0.01 for a, b in zip(Js, Js[1:]))
    assert Js[-1] >= HOST_END_J - 1e-4 and errs[-1] <= HOST_END_MM
    assert r["fitted"].all() and r["pixels"][0] > 500 and r["cam_t"].dtype == np.float32
    # what is returned folds together: placed = rotation (vertices + cam_t - pivot) + pivot', cam_t' = cam_t + pivot' - pivot
    p0 = start.astype(np.float64)
    again = np.einsum("bij,bvj->bvi", r["rotation"], verts.astype(np.float64) + p0[:, None] - p0[:, None]) + r["pivot"][:, None]
    assert np.abs(again - r["trail"][-1]).max() <= 1e-12
    assert np.abs(r["cam_t"].astype(np.float64) - r["pivot"]).max() <= 1e-7            # the pivot was the origin
    # a hand that cannot be solved stays where it is, byte for byte
    few = MR.fit_contour(render, verts, start, start.astype(np.float64), [0], mask, [SCENE["label"]], cams, rounds=2, radius=16, min_pixels=10 ** 6)
    assert few["cam_t"].tobytes() == start.tobytes() and not few["fitted"].any() and few["rotation"].tobytes() == np.eye(3)[None].tobytes()
    far = MR.fit_contour(render, verts, start, start.astype(np.float64), [0], mask, [SCENE["label"]], cams, rounds=2, radius=2)
    assert far["cam_t"].tobytes() == start.tobytes() or far["fitted"].any()


def test_directions_of_a_batch():
    assert ME.fit_directions([0, 0, 1, 2, 2], [3, 3, 3, 3, 4]) == [1, 1, 3, 3, 3]
    assert ME.fit_directions([], []) == []
    assert ME.fit_radius(1080, 1920) == 36 and ME.fit_radius(720, 1280) == 24 and ME.fit_radius(240, 320) == 8
    assert ME.fit_radius(4000, 6000) == 64 == ME.MAX_RADIUS
    assert MR.COUNT_NAMES == ME.FIT_COUNT_NAMES


# ------------------------------------------------------------------ folding a fit into a record
ROUND_TRIP_M = 2e-4                                                                    # tests/test_gpu_api.py: a record's OBJ against its vertices


def test_record_folding():
    from hamer_yolo_amd import evaluate_masks as EM
    rng = np.random.default_rng(11)
    X, J0 = rng.normal(0, 0.05, (40, 3)), np.array([0.09, 0.005, 0.006])                # a made-up hand and its wrist joint

    def mano(pose_global):                                                              # MANO turns the hand about the wrist joint
        return (X - J0) @ MR.exp_so3(np.asarray(pose_global, np.float64)[None])[0].T + J0

    cams = np.array([[600.0, 610.0, 160.0, 120.0]])
    for is_right in (True, False):
        Mx = np.diag([1.0 if is_right else -1.0, 1.0, 1.0])
        pg, ph = rng.normal(0, 0.6, 3).astype(np.float32), rng.normal(0, 0.1, 45).astype(np.float32)
        hand = {"betas": np.zeros(10, np.float32), "theta": np.concatenate([pg, ph]), "pose_hand": ph, "pose_global": pg,
                "cam_t": np.array([0.1, -0.05, 0.6], np.float32), "is_right": is_right}
        cam_t = hand["cam_t"].astype(np.float64)
        placed = (mano(pg) @ Mx + cam_t)[None]
        pivot = (Mx @ J0 + cam_t)[None]
        sol = np.array([[0.03, -0.06, 2.5, -1.25, 0.4, 1.0, 0.0, 0.0]])
        centre = MR.centre_of(MR.project(cams, [0], pivot)).astype(np.float64)
        R, pv2, moved, ok = MR.contour_step(np.eye(3)[None], pivot, placed, sol, centre, cams, [0], 16)
        assert ok.all() and abs(pv2[0, 2] - pivot[0, 2] / np.hypot(1.03, 0.06)) < 1e-15
        new_t = (cam_t + (pv2[0] - pivot[0])).astype(np.float32)
        data = {"right": hand, "left": None} if is_right else {"right": None, "left": hand}
        side = "right" if is_right else "left"
        out = EM._contour_record(data, {side: (R[0], new_t, 0.4, 321, True)})[side]
        # the record, run through MANO again, is the placed mesh
        got = mano(out["pose_global"]) @ Mx + out["cam_t"].astype(np.float64)
        assert np.abs(got - moved[0]).max() <= ROUND_TRIP_M, np.abs(got - moved[0]).max()
        assert np.abs(got - moved[0]).max() <= 1e-6                                    # float32 of pose_global and cam_t, nothing more
        assert set(out) == set(hand) | set(EM.FIT_KEYS)
        assert EM.FIT_KEYS == ("cam_t_unrefined", "pose_global_unrefined", "mask_fit_rms_px", "mask_fit_pixels", "mask_fit")
        assert out["cam_t_unrefined"] is hand["cam_t"] and out["pose_global_unrefined"] is pg
        assert out["pose_global"].dtype == np.float32 and out["cam_t"].dtype == np.float32 and out["theta"].dtype == np.float32
        assert np.array_equal(out["theta"][:3], out["pose_global"]) and np.array_equal(out["theta"][3:], ph)
        assert (out["mask_fit_rms_px"], out["mask_fit_pixels"], out["mask_fit"]) == (0.4, 321, True)
        assert np.array_equal(hand["theta"][:3], pg)                                   # the input record is left alone
        # a hand that was not fitted keeps its bytes; keys a depth refinement set already stay
        kept = EM._contour_record(data, {side: (R[0], new_t, 0.0, 3, False)})[side]
        assert kept["pose_global"] is pg and kept["cam_t"] is hand["cam_t"] and kept["theta"] is hand["theta"] and kept["mask_fit"] is False
        none = EM._contour_record(data, {})[side]
        assert np.isnan(none["mask_fit_rms_px"]) and none["mask_fit_pixels"] == 0 and none["mask_fit"] is False
        first = np.array([9.0, 9.0, 9.0], np.float32)
        two = EM._contour_record({side: dict(hand, cam_t_unrefined=first), "other": 1}, {side: (R[0], new_t, 0.4, 321, True)})
        assert two[side]["cam_t_unrefined"] is first and two["other"] == 1


# ------------------------------------------------------------------ surface
NAMES = ("hm_mask_fit_workspace_bytes", "hm_mask_fit")


def test_surface():
    header = open(os.path.join(ROOT, "include", "hamer_hip.h")).read()
    lib = L.load()
    for name in NAMES:
        assert re.search(r"\b%s\(" % name, header) and name in L.EXPORTS and hasattr(lib, name), name
    assert "mask_fit.hip" in B.SOURCES and os.path.exists(os.path.join(B.CSRC, "mask_fit.hip"))
    assert "---- Mask fit" in header and "2^18 used pixels" in header and "llrint((double)(Jr_i Jr_j) / (double)d2 * 2^20)" in header
    assert int(re.search(r"#define HM_VERSION (\d+)", header).group(1)) == L.HM_VERSION == lib.hm_version() == 402
    src = open(os.path.join(B.CSRC, "mask_fit.hip")).read()
    assert "#pragma clang fp contract(off)" in src
    for word in ("getenv", "hipMalloc", "asm", "hipDeviceSynchronize", "hipStreamSynchronize", "printf"):
        assert word not in src, word
    assert lib.hm_mask_fit_workspace_bytes.restype is C.c_size_t and len(lib.hm_mask_fit.argtypes) == 20
    assert "hm_mask_fit" not in open(os.path.join(B.CSRC, "mask_eval.hip")).read()      # the scores' unit is left alone


def test_workspace_bytes():
    lib = L.load()
    for Q in (1, 2, 3, 16, 256):
        assert lib.hm_mask_fit_workspace_bytes(Q, 1080, 1920, 36) == Q * (2 * 1080 * 30 + 32) * 8
    assert lib.hm_mask_fit_workspace_bytes(3, 37, 53, 3) == 3 * (2 * 37 + 32) * 8
    assert lib.hm_mask_fit_workspace_bytes(0, 37, 53, 3) == (2 * 37 + 32) * 8
    assert lib.hm_mask_fit_workspace_bytes(4, 70, 131, 5) == lib.hm_mask_fit_workspace_bytes(4, 70, 131, 64)
    for bad in ((-1, 4, 4, 1), (1, 0, 4, 1), (1, 4, 0, 1), (1, 4, 4, -1), (1, 4, 4, 65)):
        assert lib.hm_mask_fit_workspace_bytes(*bad) == 0, bad


ORDER = ("pred_id", "mask", "N", "H", "W", "queries", "Q", "centre", "radius", "reach_px", "directions", "damping", "lever_px",
         "min_pixels", "sums", "counts", "solution", "workspace", "workspace_bytes", "stream")


def _call(**kw):
    """hm_mask_fit over MADE-UP device addresses that are never dereferenced: every case below must fail in the host part,
    before any launch."""
    a = dict(pred_id=0x20000, mask=0x40000, N=2, H=37, W=53, queries=0x60000, Q=3, centre=0x70000, radius=5, reach_px=4096,
             directions=3, damping=1e-3, lever_px=50.0, min_pixels=30, sums=0x90000, counts=0xA0000, solution=0xB0000,
             workspace=0xC0000, workspace_bytes=None, stream=None)
    a.update(kw)
    lib = L.load()
    if a["workspace_bytes"] is None:
        a["workspace_bytes"] = max(int(lib.hm_mask_fit_workspace_bytes(max(a["Q"], 0), max(a["H"], 1), max(a["W"], 1), 3)), 8)
    rc = lib.hm_mask_fit(*[a[k] for k in ORDER])
    return rc, lib.hm_last_error_string().decode()


INF, NAN = float("inf"), float("nan")


ARG_CASES = [
    (dict(pred_id=None), "null"), (dict(mask=None), "null"), (dict(queries=None), "null"), (dict(centre=None), "null"),
    (dict(sums=None), "null"), (dict(counts=None), "null"), (dict(solution=None), "null"), (dict(workspace=None), "null"),
    (dict(N=0), "positive"), (dict(H=0), "positive"), (dict(W=-1), "positive"), (dict(N=1024, H=1024, W=2048), "2^31"),
    (dict(N=2, H=32768, W=32768), "2^31"), (dict(Q=-1), "negative"),
    (dict(radius=-1), "radius"), (dict(radius=65), "radius"), (dict(reach_px=0), "reach_px"), (dict(reach_px=4097), "reach_px"),
    (dict(directions=0), "directions"), (dict(directions=4), "directions"), (dict(directions=-1), "directions"),
    (dict(damping=-1e-9), "damping"), (dict(damping=INF), "damping"), (dict(damping=NAN), "damping"),
    (dict(lever_px=0.0), "lever_px"), (dict(lever_px=-5.0), "lever_px"), (dict(lever_px=INF), "lever_px"), (dict(lever_px=NAN), "lever_px"),
    (dict(min_pixels=0), "min_pixels"), (dict(min_pixels=-5), "min_pixels"),
    (dict(workspace_bytes=0), "workspace"), (dict(workspace_bytes=3 * (2 * 37 + 32) * 8 - 1), "workspace"),
    (dict(sums=0x90004), "aligned"), (dict(counts=0xA0004), "aligned"), (dict(solution=0xB0004), "aligned"),
    (dict(workspace=0xC0004), "aligned"), (dict(pred_id=0x20002), "aligned"), (dict(queries=0x60002), "aligned"),
    (dict(centre=0x70002), "aligned"),
]


@pytest.mark.parametrize("kw,word", ARG_CASES)
def test_argument_checks(kw, word):
    rc, msg = _call(**kw)
    assert rc == -1 and "hm_mask_fit" in msg and word in msg, (rc, msg)                 # HM_ERR_ARG


def test_no_queries_and_limits_pass_the_checks_without_a_launch():
    assert _call(Q=0)[0] == 0
    assert _call(Q=0, queries=None, centre=None, sums=None, counts=None, solution=None, workspace=None, workspace_bytes=0)[0] == 0
    assert _call(Q=0, radius=0, reach_px=1, directions=1, damping=0.0, min_pixels=1)[0] == 0     # the ends of the ranges are legal
    assert _call(Q=0, radius=64, reach_px=4096, directions=3)[0] == 0


# ------------------------------------------------------------------ the Python layer and the drivers
def test_python_layer_raises_without_a_gpu_and_on_bad_inputs():
    i, m = torch.zeros(1, 4, 5, dtype=torch.int32), torch.zeros(1, 4, 5, dtype=torch.uint8)
    with pytest.raises(ValueError, match="GPU"):
        ME.mask_fit(i, m, [(0, 0, 1, 3)], [(2, 2)], radius=3)
    with pytest.raises(ValueError):
        ME.mask_fit(i.numpy(), m.numpy(), [(0, 0, 1, 3)], [(2, 2)], radius=3)
    p = inspect.signature(ME.mask_fit).parameters
    assert list(p) == ["pred_id", "mask", "queries", "centre", "radius", "reach_px", "directions", "damping", "lever_px", "min_pixels"]
    assert p["radius"].default is inspect.Parameter.empty and all(p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(p)[4:])
    p = inspect.signature(ME.fit_contour).parameters
    assert list(p)[:11] == ["H", "W", "K", "vertices", "faces", "cam_t", "pivot", "frame_index", "mask", "labels", "rounds"]
    assert p["rounds"].default == 6 and p["radius"].default is None and p["max_rot_rad"].default == 0.5 and p["max_scale"].default == 2.0
    with pytest.raises(ValueError, match="GPU"):
        ME.fit_contour(4, 5, np.eye(3), torch.zeros(1, 3, 3), [[0, 1, 2]], torch.zeros(1, 3), torch.zeros(1, 3), [0], m, [3])
    assert ME._fit_ws == {} and ME.release_fit_workspaces() is None


def test_driver_parsers():
    from hamer_yolo_amd import d_infer, infer
    from hamer_yolo_amd import evaluate_masks as EM
    base = ["--pred", "A", "--images", "B", "--masks", "C"]
    a = EM._parser().parse_args(base)
    assert a.refine_to is None and a.fit_rounds == 6 and a.fit_radius is None
    a = EM._parser().parse_args(base + ["--refine-to", "R", "--fit-rounds", "3", "--fit-radius", "20"])
    assert (a.refine_to, a.fit_rounds, a.fit_radius) == ("R", 3, 20)
    for bad in (["--fit-rounds", "3"], ["--fit-radius", "9"], ["--refine-to", "R", "--fit-radius", "65"]):
        with pytest.raises(SystemExit) as e:
            EM.main(base + bad)
        assert e.value.code == 2
    p = inspect.signature(EM.refine_folder).parameters
    assert list(p)[:6] == ["image_folder", "npy_folder", "mask_folder", "out_folder", "hamer", "k_real"] and p["rounds"].default == 6
    a = infer._parser().parse_args(["--input", "A", "--output", "B"])
    assert a.mask_fit == "none" and a.masks is None
    a = infer._parser().parse_args(["--input", "A", "--output", "B", "--masks", "M", "--mask-fit", "contour"])
    assert (a.masks, a.mask_fit) == ("M", "contour")
    with pytest.raises(SystemExit) as e:
        infer.main(["--input", "A", "--output", "B", "--mask-fit", "contour"])          # needs --masks
    assert e.value.code == 2
    with pytest.raises(SystemExit):
        infer._parser().parse_args(["--input", "A", "--output", "B", "--masks", "M", "--mask-fit", "affine"])
    assert "the mask fit runs first" in " ".join(infer._parser().format_help().split())
    a = d_infer._parser().parse_args(["--input", "A", "--output", "B", "--intrinsics", "K"])
    assert a.mask_fit == "none" and a.masks is None
    a = d_infer._parser().parse_args(["--input", "A", "--output", "B", "--intrinsics", "K", "--masks", "M", "--mask-fit", "contour"])
    assert (a.masks, a.mask_fit) == ("M", "contour")
    with pytest.raises(SystemExit) as e:
        d_infer.main(["--input", "A", "--output", "B", "--intrinsics", "K", "--mask-fit", "contour"])
    assert e.value.code == 2
