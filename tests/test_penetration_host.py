"""Host checks of the interpenetration rule (tests/penetration_rule.py, stated in include/hamer_hip.h "Penetration"): the inside
test against analytic solids and against the generalised winding number, the distance against the analytic signed distance of a
box, two inscribed spheres, close_boundaries, statuses and invalid data, the resolve loop, and the surface: prototypes, exports,
argument checks through ctypes, the drivers' parsers and the record fold.  No GPU."""
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
import penetration_rule as PR  # noqa: E402

from hamer_yolo_amd import build as B  # noqa: E402
from hamer_yolo_amd import lib as L  # noqa: E402
from hamer_yolo_amd.hamer.utils import penetration as PN  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q = 1.0 / 65536.0                                                          # one quantum in metres


# ------------------------------------------------------------------ constructed meshes
def box_mesh(lo, hi):
    """The twelve triangles of an axis-aligned box, outward."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    v = np.array([[(lo, hi)[(i >> k) & 1][k] for k in range(3)] for i in range(8)], np.float64)
    f = [(0, 2, 3), (0, 3, 1), (4, 5, 7), (4, 7, 6), (0, 1, 5), (0, 5, 4), (2, 6, 7), (2, 7, 3), (0, 4, 6), (0, 6, 2), (1, 3, 7), (1, 7, 5)]
    return v, np.asarray(f, np.int32)


def octahedron(R):
    v = np.array([[R, 0, 0], [-R, 0, 0], [0, R, 0], [0, -R, 0], [0, 0, R], [0, 0, -R]], np.float64)
    f = [(0, 2, 4), (2, 1, 4), (1, 3, 4), (3, 0, 4), (2, 0, 5), (1, 2, 5), (3, 1, 5), (0, 3, 5)]
    return v, np.asarray(f, np.int32)


def lattice(lo, hi):
    """Every integer point of [lo, hi]^3, in metres: the lattice of the rule's fixed point."""
    r = np.arange(lo, hi + 1)
    return np.stack(np.meshgrid(r, r, r, indexing="ij"), -1).reshape(-1, 3).astype(np.float64) * Q


def star(n_lat=10, n_lon=16, scale=0.05):
    """A deliberately non-convex closed mesh: the unit sphere's lat-lon mesh with four lobes pushed out and in."""
    v, f = DR.ellipsoid((1.0, 1.0, 1.0), n_lat=n_lat, n_lon=n_lon)
    r = 1.0 + 0.45 * np.cos(4.0 * np.arctan2(v[:, 1], v[:, 0])) * (1.0 - v[:, 2] ** 2)
    return v * r[:, None] * scale, f


def winding(points, verts, faces):
    """The generalised winding number (Van Oosterom and Strackee's solid angles, float64): 1 inside a closed outward mesh."""
    a, b, c = (verts[faces[:, k]][None] - points[:, None] for k in range(3))
    la, lb, lc = (np.linalg.norm(x, axis=2) for x in (a, b, c))
    num = np.einsum("pfk,pfk->pf", a, np.cross(b, c))
    den = la * lb * lc + np.einsum("pfk,pfk->pf", a, b) * lc + np.einsum("pfk,pfk->pf", b, c) * la + np.einsum("pfk,pfk->pf", c, a) * lb
    return (2.0 * np.arctan2(num, den)).sum(1) / (4.0 * np.pi)


def snapped(x):
    """x on the rule's lattice, in metres: quantise first, then compare."""
    return np.rint(np.asarray(x, np.float64) * 65536.0) * Q


def rule_distance(r):
    """The rule's unsigned distance in float64 metres (NaN where a vertex has none): its float32 output is too coarse for 1e-12."""
    d = np.sqrt((r["delta"] ** 2).sum(1)) * Q
    return np.where(r["nearest_face"] >= 0, d, np.nan)


# ------------------------------------------------------------------ the inside test
@pytest.mark.parametrize("solid", ["cube", "octahedron"])
def test_inside_on_every_lattice_point(solid):
    """Rays through edges, vertices and (for the cube) along vertical faces included; points ON the surface are the rule's to
    define and are left out."""
    if solid == "cube":
        v, f = box_mesh((0, 0, 0), (4 * Q, 4 * Q, 4 * Q))
        pts = lattice(-2, 6)
        X = np.rint(pts / Q)
        inside = ((X > 0) & (X < 4)).all(1)
        on = ((X >= 0) & (X <= 4)).all(1) & ~inside
    else:
        v, f = octahedron(4 * Q)
        pts = lattice(-6, 6)
        s = np.abs(np.rint(pts / Q)).sum(1)
        inside, on = s < 4, s == 4
    r = PR.query(pts, v, f, contact_tol_m=2 * Q)
    assert r["sums"][PR.STATUS] == PR.OK and inside.sum() > 20 and (~inside & ~on).sum() > 200
    got = r["code"] == PR.INSIDE
    assert np.array_equal(got[~on], inside[~on])
    assert r["sums"][PR.N_INSIDE] == got.sum() and (r["signed_distance"][inside] < 0).all()
    for order in ([0, 2, 1], [1, 2, 0]):                                   # the winding of b does not matter, nor its corner order
        again = PR.query(pts, v, f[:, order], contact_tol_m=2 * Q)
        assert np.array_equal(again["code"], r["code"])


@pytest.mark.parametrize("shape", ["ellipsoid", "star"])
def test_inside_against_the_winding_number(shape):
    v, f = DR.ellipsoid((0.05, 0.08, 0.02), n_lat=10, n_lon=16) if shape == "ellipsoid" else star()
    rng = np.random.default_rng(7)
    v = snapped(v + (0.01, -0.02, 0.5))
    pts = snapped(rng.uniform(v.min(0) - 0.005, v.max(0) + 0.005, (1500, 3)))
    r = PR.query(pts, v, f, contact_tol_m=0.01)
    w = winding(pts, v, f)
    keep = ~(rule_distance(r) < 1e-6)                                      # at least 1e-6 m from the surface
    assert keep.sum() > 1400 and (np.abs(w[keep] - np.rint(w[keep])) < 1e-6).all()
    assert np.array_equal((r["code"] == PR.INSIDE)[keep], (w > 0.5)[keep])
    assert 200 < (w > 0.5).sum() < 1300
    n = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    in_front = np.einsum("fk,vfk->vf", n, v[:, None, :] - v[f[:, 0]][None]) > 1e-4       # a vertex 0.1 mm beyond a face's plane: not convex
    assert in_front.any() == (shape == "star")


# ------------------------------------------------------------------ the distance
def box_sdf(p, lo, hi):
    c, h = (lo + hi) / 2, (hi - lo) / 2
    q = np.abs(p - c) - h
    return np.linalg.norm(np.maximum(q, 0.0), axis=1) + np.minimum(q.max(1), 0.0)


def test_distance_against_the_analytic_box():
    lo, hi = snapped((-0.03, 0.01, 0.4)), snapped((0.05, 0.07, 0.52))
    v, f = box_mesh(lo, hi)
    rng = np.random.default_rng(11)
    inside = rng.uniform(lo, hi, (300, 3))
    around = rng.uniform(lo - 0.03, hi + 0.03, (600, 3))
    pick = lambda k: np.where(rng.random((200, 3)) < 0.5, lo, hi) + rng.uniform(-0.02, 0.02, (200, 3)) * (np.arange(3) != k)   # noqa: E731
    edges = np.concatenate([np.where(np.arange(3) == k, rng.uniform(lo, hi, (200, 3)), pick(k) + rng.uniform(0, 0.02, (200, 3)) *
                                     np.where(rng.random((200, 3)) < 0.5, -1, 1)) for k in range(3)])
    corners = np.where(rng.random((300, 3)) < 0.5, lo - rng.uniform(0, 0.03, (300, 3)), hi + rng.uniform(0, 0.03, (300, 3)))
    exact = np.array([lo, hi, (lo + hi) / 2, [lo[0], hi[1], (lo[2] + hi[2]) / 2]])          # corners, the centre, a point on an edge
    pts = snapped(np.concatenate([inside, around, edges, corners, exact]))
    want = box_sdf(pts, lo, hi)
    r = PR.query(pts, v, f, contact_tol_m=0.06)
    assert r["sums"][PR.TESTED] == len(pts) and (r["nearest_face"] >= 0).all()
    got = rule_distance(r) * np.where(r["code"] == PR.INSIDE, -1.0, 1.0)
    off = want != 0
    assert np.array_equal((r["code"] == PR.INSIDE)[off], (want < 0)[off])
    err = np.abs(np.abs(got) - np.abs(want))
    print("box distance: max error %.3g m over %d points" % (err.max(), len(pts)))
    assert err.max() <= 1e-12
    assert np.array_equal(r["signed_distance"], got.astype(np.float32))
    regions = (np.abs(pts - (lo + hi) / 2) > (hi - lo) / 2).sum(1)        # 0 inside, 1 face, 2 edge, 3 corner regions
    assert all((regions == k).sum() > 50 for k in range(4))
    # the counts and the sums are those of the vertex outputs
    ins = r["code"] == PR.INSIDE
    d = rule_distance(r)
    assert r["sums"][PR.N_INSIDE] == ins.sum() and r["sums"][PR.N_NEAR] == (r["code"] == PR.NEAR).sum()
    assert PR.max_depth(r["sums"]) == d[ins].max() and r["sums"][PR.SUM_DEPTH] == np.rint(d[ins] * 2.0 ** 32).astype(np.int64).sum()
    assert np.array_equal(r["sums"][PR.PUSH_X:], np.rint(r["delta"][ins] * 65536.0).astype(np.int64).sum(0))


def sphere_pair(r=0.05, c=0.07, n_lat=12, n_lon=24):
    v, f = DR.ellipsoid((r, r, r), n_lat=n_lat, n_lon=n_lon)
    return v + (0.0, 0.0, 0.5), v + (0.0, 0.0, 0.5 + c), f


def sphere_bound(r, n_lat, n_lon):
    """How far an inscribed lat-lon mesh can lie inside its sphere: no point of a face is further from its corners than half
    the face's angular diagonal phi <= sqrt(dlat^2 + dlon^2) / 2, so the face stays within r (1 - cos phi) of the sphere."""
    phi = 0.5 * np.hypot(np.pi / n_lat, 2.0 * np.pi / n_lon)
    return r * (1.0 - np.cos(phi))


def test_two_inscribed_spheres():
    """The pole of a lies on the line of centres, 2r - c inside b's sphere.  b's mesh lies inside that sphere by at most h, so
    the pole's depth is in [2r - c - h, 2r - c], and no vertex of a is deeper inside the sphere than the pole: the maximum depth
    lies in the same interval, up to the quantisation of the vertices (two quanta cover a and b)."""
    r, c, n_lat, n_lon = 0.05, 0.07, 12, 24
    va, vb, f = sphere_pair(r, c, n_lat, n_lon)
    h = sphere_bound(r, n_lat, n_lon)
    for a, b in ((va, vb), (vb, va)):
        out = PR.query(a, b, f)
        d = PR.max_depth(out["sums"])
        print("two spheres: depth %.6f m, 2r - c = %.6f m, polyhedral bound %.6f m" % (d, 2 * r - c, h))
        assert 2 * r - c - h - 2 * Q <= d <= 2 * r - c + 2 * Q and h < 0.001
        assert out["sums"][PR.N_INSIDE] > 10 and out["sums"][PR.STATUS] == PR.OK
        s = PN.summary(out["sums"][None])
        assert s["max_depth_m"][0] == d and 0 < s["mean_depth_m"][0] < d and s["inside"][0] == out["sums"][PR.N_INSIDE]
        push = out["sums"][PR.PUSH_X:].astype(np.float64)
        assert abs(push[2]) > 100 * max(abs(push[0]), abs(push[1])) and (push[2] < 0) == (a is va)     # a leaves b along the axis


# ------------------------------------------------------------------ close_boundaries
def edge_uses(f):
    e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), 1)
    return np.unique(e, axis=0, return_counts=True)[1]


@pytest.mark.parametrize("close", [PR.close_boundaries, PN.close_boundaries])
def test_close_boundaries(close):
    v, f = DR.ellipsoid((0.05, 0.08, 0.02), n_lat=8, n_lon=12)
    assert close(f, len(v)).shape == (0, 3) and close(f, len(v)).dtype == np.int32        # closed already
    top, bottom = (f == 0).any(1), (f == len(v) - 1).any(1)
    cut = f[~top]                                                          # the cap around the first pole is gone
    extra = close(cut, len(v))
    assert len(extra) == 12 - 2 and (edge_uses(cut) == 1).sum() == 12
    assert extra[:, 0].tolist() == [1] * 10                                # one loop, fanned from its lowest vertex
    closed = np.concatenate([cut, extra])
    assert (edge_uses(closed) == 2).all()
    vq = snapped(v + (0.0, 0.0, 0.5))
    pts = snapped(np.random.default_rng(3).uniform(vq.min(0) - 0.004, vq.max(0) + 0.004, (800, 3)))
    r = PR.query(pts, vq, closed, contact_tol_m=0.01)
    w = winding(pts, vq, closed)                                           # > 0: the fan faces outward with the rest
    keep = ~(rule_distance(r) < 1e-6)
    assert np.array_equal((r["code"] == PR.INSIDE)[keep], (w > 0.5)[keep]) and (np.abs(w[keep] - np.rint(w[keep])) < 1e-6).all()
    assert 100 < (w > 0.5).sum() < 700
    two = close(f[~top & ~bottom], len(v))                                 # two holes, two fans
    assert len(two) == 20 and sorted(set(two[:, 0].tolist())) == [1, len(v) - 13]
    assert (edge_uses(np.concatenate([f[~top & ~bottom], two])) == 2).all()
    assert np.array_equal(PN.closed_faces(cut, len(v)), closed)
    with pytest.raises(ValueError):
        close(np.array([[0, 1, 9]]), 3)


# ------------------------------------------------------------------ statuses and invalid data
def test_statuses_and_invalid_data():
    va, vb, f = sphere_pair(n_lat=6, n_lon=8)
    base = PR.query(va, vb, f)
    assert base["sums"][PR.STATUS] == PR.OK and base["sums"][PR.N_INSIDE] > 0
    # TOO_LARGE: a box side of 2 m, in a or in b; one quantum less is fine
    for big_a in (True, False):
        wide = (va if big_a else vb).copy()
        wide[1, 0] = wide[:, 0].min() + 2.0
        r = PR.query(wide, vb, f) if big_a else PR.query(va, wide, f)
        assert r["sums"].tolist() == [0, 0, 0, 0, PR.TOO_LARGE, 0, 0, 0, 0, 0]
        assert (r["code"] == PR.INVALID).all() and np.isnan(r["signed_distance"]).all() and (r["nearest_face"] == -1).all()
    ok = vb.copy()
    ok[1, 0] = snapped(ok[:, 0].min()) + 2.0 - Q
    assert PR.query(va, ok, f)["sums"][PR.STATUS] == PR.OK
    # NaN and infinite vertices of a are INVALID and change no one else's answer
    bad = va.copy()
    bad[3, 1], bad[5, 2], bad[7, 0] = np.nan, np.inf, 16384.0
    r = PR.query(bad, vb, f)
    rest = np.ones(len(va), bool)
    rest[[3, 5, 7]] = False
    assert r["code"][~rest].tolist() == [PR.INVALID] * 3 and np.isnan(r["signed_distance"][~rest]).all() and r["sums"][PR.N_INVALID] == 3
    assert np.array_equal(r["code"][rest], base["code"][rest]) and np.array_equal(r["signed_distance"][rest], base["signed_distance"][rest])
    # a NaN vertex of b, and a corner index out of range, drop the faces that name them: the rule equals the mesh without them
    holed = vb.copy()
    holed[9] = np.nan
    names9 = (f == 9).any(1)
    r, want = PR.query(va, holed, f), PR.query(va, vb, np.where(names9[:, None], -1, f))
    assert all(np.array_equal(r[k], want[k], equal_nan=True) for k in ("code", "signed_distance", "nearest_face", "sums"))
    wild = f.copy()
    wild[4, 1], wild[6, 2] = len(vb), -1
    r, want = PR.query(va, vb, wild), PR.query(va, vb, np.where((np.arange(len(f))[:, None] == 4) | (np.arange(len(f))[:, None] == 6), -1, f))
    assert all(np.array_equal(r[k], want[k], equal_nan=True) for k in ("code", "signed_distance", "nearest_face", "sums"))
    # zero-area faces (a repeated corner, three collinear corners) are skipped: appended to b they change nothing
    more = np.concatenate([f, [[2, 2, 5], [1, 1, 1], [2, len(vb), 5]]]).astype(np.int32)
    r = PR.query(va, np.concatenate([vb, vb[2:3]]), more)                  # the new vertex coincides with vertex 2
    assert all(np.array_equal(r[k], base[k], equal_nan=True) for k in ("code", "signed_distance", "nearest_face", "sums"))
    bv, bf = box_mesh((0, 0, 0), (8 * Q, 8 * Q, 8 * Q))
    i0, i1 = 0, int(np.nonzero((bv == (8 * Q, 0, 0)).all(1))[0][0])
    mid = np.concatenate([bv, [[4 * Q, 0.0, 0.0]]])                        # on the edge between corners i0 and i1: three distinct collinear corners
    pts = lattice(-2, 10)
    r, want = PR.query(pts, mid, np.concatenate([bf, [[i0, 8, i1]]]).astype(np.int32), 2 * Q), PR.query(pts, bv, bf, 2 * Q)
    assert all(np.array_equal(r[k], want[k], equal_nan=True) for k in ("code", "signed_distance", "nearest_face", "sums"))
    # disjoint boxes: FAR, no face read (faces that would raise if indexed are never looked at), invalid still counted
    far = vb + (0.0, 0.0, 0.2)
    r = PR.query(bad, far, f)
    assert r["sums"].tolist() == [0, 0, 0, 3, PR.DISJOINT, 0, 0, 0, 0, 0]
    assert (r["code"][rest] == PR.FAR).all() and np.isinf(r["signed_distance"][rest]).all() and (r["nearest_face"] == -1).all()
    assert PR.query(va, np.full((4, 3), np.nan), f[:2])["sums"][PR.STATUS] == PR.DISJOINT      # b without a valid vertex
    assert PR.query(np.zeros((0, 3)), vb, f)["sums"][PR.STATUS] == PR.DISJOINT                 # a without vertices
    # the boxes overlap but a vertex outside b's inflated box is FAR untested
    r = PR.query(va, vb, f, contact_tol_m=0.001)
    outside = (np.rint(va * 65536) < np.rint(vb * 65536).min(0) - 66).any(1)
    assert outside.sum() > 5 and (r["code"][outside] == PR.FAR).all() and r["sums"][PR.TESTED] == (~outside).sum()
    # a mesh against itself shifted by one quantum: every vertex is tested and lies within a quantum's diagonal of the surface
    r = PR.query(snapped(va) + (Q, 0.0, 0.0), va, f, contact_tol_m=0.001)
    assert r["sums"][PR.TESTED] == len(va) and r["sums"][PR.N_INSIDE] + r["sums"][PR.N_NEAR] == len(va)
    assert np.nanmax(rule_distance(r)) <= Q * (1 + 1e-9) and 0 < r["sums"][PR.N_INSIDE] < len(va)


# ------------------------------------------------------------------ resolve
OVERSHOOT_MEASURED_M = 0.003447265625                                      # measured on the CPU with gain 1.125: r = 0.05, c = 0.07, 12 x 24


def test_resolve_loop_on_two_spheres():
    """The measure-then-move loop through the rule: no vertex inside afterwards, the hands moved along the line of centres, and
    the overshoot past 2r - c as measured on the CPU for gain 1.125 plus a margin of 10 %."""
    r, c = 0.05, 0.07
    va, vb, f = sphere_pair(r, c)
    shift, last = PR.resolve([va, vb], [f, f], [(0, 1)], rounds=8, gain=PN.GAIN)
    assert last[0, :, PR.N_INSIDE].tolist() == [0, 0]
    apart = shift[1] - shift[0]
    over = apart[2] - (2 * r - c)
    print("resolve: moved apart by %.6f m along z (%.2e, %.2e across), overshoot past 2r - c %.6f m" % (apart[2], apart[0], apart[1], over))
    assert abs(apart[0]) < 1e-4 and abs(apart[1]) < 1e-4 and np.allclose(shift[0], -shift[1], atol=2 * Q)
    assert -sphere_bound(r, 12, 24) - 4 * Q <= over <= OVERSHOOT_MEASURED_M * 1.1
    # already apart: nothing moves
    shift, last = PR.resolve([va, vb + (0, 0, 0.2)], [f, f], [(0, 1)], rounds=2)
    assert not shift.any() and last[0, :, PR.STATUS].tolist() == [PR.DISJOINT] * 2


# ------------------------------------------------------------------ surface
NAMES = ("hm_mesh_penetration_workspace_bytes", "hm_mesh_penetration")
ORDER = ("verts", "n_verts", "faces", "n_faces", "meshes", "n_meshes", "queries", "n_queries", "contact_tol_m", "code", "signed_distance",
         "nearest_face", "n_rows", "sums", "workspace", "workspace_bytes", "stream")


def test_surface():
    header = open(os.path.join(ROOT, "include", "hamer_hip.h")).read()
    lib = L.load()
    for name in NAMES:
        assert re.search(r"\b%s\(" % name, header) and name in L.EXPORTS and hasattr(lib, name), name
    assert "penetration.hip" in B.SOURCES and os.path.exists(os.path.join(B.CSRC, "penetration.hip"))
    assert "---- Penetration" in header and "Exactness." in header and "ties to the lower face row" in header
    assert int(re.search(r"#define HM_VERSION (\d+)", header).group(1)) == L.HM_VERSION == lib.hm_version()
    src = open(os.path.join(B.CSRC, "penetration.hip")).read()
    assert "#pragma clang fp contract(off)" in src
    for word in ("getenv", "hipMalloc", "asm", "hipDeviceSynchronize", "hipStreamSynchronize", "printf"):
        assert word not in src, word
    assert lib.hm_mesh_penetration_workspace_bytes.restype is C.c_size_t and len(lib.hm_mesh_penetration.argtypes) == len(ORDER)
    assert C.sizeof(L.PenQuery) == 8 and re.search(r"hm_pen_query \{ int32_t a, b; \}", header)
    assert PN.CODES == ("FAR", "NEAR", "INSIDE", "INVALID") and PN.STATUSES == ("OK", "DISJOINT", "TOO_LARGE")
    for i, name in enumerate(PN.CODES):
        assert re.search(r"HM_PEN_%s = %d\b" % (name, i), header) and getattr(PN, name) == getattr(PR, name) == i
    for i, name in enumerate(PN.STATUSES):
        assert re.search(r"HM_PEN_%s = %d\b" % (name, i), header) and getattr(PR, name) == i
    assert [PN.SUM_NAMES.index(n) for n in ("tested", "near", "inside", "invalid", "status", "max_depth_bits", "sum_depth", "push_x")] == \
        [PR.TESTED, PR.N_NEAR, PR.N_INSIDE, PR.N_INVALID, PR.STATUS, PR.MAX_BITS, PR.SUM_DEPTH, PR.PUSH_X]
    ws = lib.hm_mesh_penetration_workspace_bytes
    assert ws(-1, 1, 1) == 0 and ws(1, -1, 1) == 0 and ws(1, 1, -1) == 0 and ws(0, 0, 0) % 256 == 0
    assert 778 * 512 * 16 <= ws(778 * 512, 512, 512) < 778 * 512 * 16 + 512 * 64 + 4096


def _table(v0=0, nv=10, f0=0, nf=12, frame=0):
    t = (L.Mesh * 2)()
    t[0].frame, t[0].v0, t[0].nv, t[0].f0, t[0].nf = frame, v0, nv, f0, nf
    t[1].frame, t[1].v0, t[1].nv, t[1].f0, t[1].nf = 1, 10, 10, 12, 8
    return t


def _queries(*pairs):
    t = (L.PenQuery * len(pairs))()
    for q, (a, b) in enumerate(pairs):
        t[q].a, t[q].b = a, b
    return t


def _call(**kw):
    """hm_mesh_penetration over MADE-UP device addresses that are never dereferenced: every case must fail in the host part."""
    a = dict(verts=0x30000, n_verts=20, faces=0x40000, n_faces=20, meshes=_table(), n_meshes=2, queries=_queries((0, 1), (1, 0)), n_queries=2,
             contact_tol_m=0.002, code=0x50000, signed_distance=0x60000, nearest_face=0x70000, n_rows=20, sums=0x80000, workspace=0xA0000,
             workspace_bytes=None, stream=None)
    a.update(kw)
    lib = L.load()
    if a["workspace_bytes"] is None:
        a["workspace_bytes"] = int(lib.hm_mesh_penetration_workspace_bytes(20, 2, 2))
    rc = lib.hm_mesh_penetration(*[a[k] for k in ORDER])
    return rc, lib.hm_last_error_string().decode()


@pytest.mark.parametrize("kw,word", [
    (dict(verts=None), "null"), (dict(faces=None), "null"), (dict(meshes=None), "null"), (dict(queries=None), "null"), (dict(sums=None), "null"),
    (dict(workspace=None), "null"), (dict(code=None), "null output"), (dict(signed_distance=None), "null output"),
    (dict(nearest_face=None), "null output"), (dict(n_meshes=-1), "negative"), (dict(n_verts=-1), "negative"), (dict(n_faces=-1), "negative"),
    (dict(n_queries=-1), "negative"), (dict(n_rows=-1), "negative"), (dict(contact_tol_m=-0.001), "contact_tol_m"),
    (dict(contact_tol_m=1.5), "contact_tol_m"), (dict(contact_tol_m=float("nan")), "contact_tol_m"), (dict(contact_tol_m=float("inf")), "contact_tol_m"),
    (dict(verts=0x30004), "aligned"), (dict(sums=0x80004), "aligned"), (dict(workspace=0xA0008), "aligned"), (dict(faces=0x40002), "aligned"),
    (dict(signed_distance=0x60002), "aligned"), (dict(nearest_face=0x70002), "aligned"),
    (dict(workspace_bytes=0), "workspace too small"), (dict(n_rows=19), "n_rows"),
    (dict(queries=_queries((0, 2), (1, 0))), "outside the table"), (dict(queries=_queries((0, 1), (-1, 0))), "outside the table"),
    (dict(meshes=_table(nv=11)), "share vertices"), (dict(meshes=_table(nf=13)), "share faces"), (dict(meshes=_table(v0=-1)), "negative mesh range"),
    (dict(meshes=_table(frame=-1)), "frame outside"), (dict(n_verts=19), "outside the vertex or face array"),
])
def test_argument_checks(kw, word):
    rc, msg = _call(**kw)
    assert rc == -1 and "hm_mesh_penetration" in msg and word in msg, (rc, msg)          # HM_ERR_ARG


def test_nothing_to_do_passes_the_checks_without_a_launch():
    assert _call(n_queries=0)[0] == 0
    assert _call(n_queries=0, verts=None, faces=None, meshes=None, queries=None, code=None, signed_distance=None, nearest_face=None, sums=None,
                 workspace=None, workspace_bytes=0, n_verts=0, n_faces=0, n_meshes=0, n_rows=0)[0] == 0


def test_python_layer_raises_without_a_gpu_and_on_bad_inputs():
    v, f = octahedron(0.01)
    meshes = [{"frame": 0, "vertices": torch.from_numpy(v), "faces": torch.from_numpy(f)}] * 2
    with pytest.raises(ValueError, match="GPU"):
        PN.mesh_penetration(meshes, [(0, 1)])
    with pytest.raises(ValueError, match="GPU"):
        PN.resolve_penetration(meshes, [(0, 1)])
    with pytest.raises(ValueError, match="outside"):
        PN.mesh_penetration(meshes, [(0, 2)])
    with pytest.raises(ValueError, match="contact_tol_m"):
        PN.mesh_penetration(meshes, [(0, 1)], contact_tol_m=-1.0)
    with pytest.raises(ValueError, match="gain"):
        PN.resolve_penetration(meshes, [(0, 1)], gain=0.0)
    assert list(inspect.signature(PN.mesh_penetration).parameters) == ["meshes", "pairs", "contact_tol_m", "stream"]
    p = inspect.signature(PN.resolve_penetration).parameters
    assert p["rounds"].default == 8 and p["gain"].default == PN.GAIN == inspect.signature(PR.resolve).parameters["gain"].default
    frames = [{"frame": k} for k in (0, 0, 1, 2, 2, 3, 3, 3)]
    assert PN.hand_pairs(frames) == [(0, 1), (3, 4)]
    s = PN.summary(np.zeros((0, 10), np.int64))
    assert s["max_depth_m"].shape == (0,) and s["inside"].dtype == np.int64


def test_driver_parsers_and_defaults():
    from hamer_yolo_amd import d_infer, infer
    from hamer_yolo_amd import evaluate_penetration as EP
    a = EP._parser().parse_args(["--pred", "p"])
    assert (a.contact_tol_mm, a.write_to, a.resolve_to, a.rounds, a.json, a.ckpt) == (2.0, None, None, 8, None, None)
    a = EP._parser().parse_args(["--pred", "p", "--contact-tol-mm", "1.5", "--write-to", "w", "--resolve-to", "r", "--rounds", "3", "--json", "j"])
    assert (a.contact_tol_mm, a.write_to, a.resolve_to, a.rounds, a.json) == (1.5, "w", "r", 3, "j")
    for bad in (["--pred", "p", "--rounds", "3"], ["--pred", "p", "--contact-tol-mm", "-1"], ["--contact-tol-mm", "2"],
                ["--pred", "p", "--resolve-to", "r", "--rounds", "-1"]):
        with pytest.raises(SystemExit):
            EP.main(bad)
    for ap in (infer._parser(), d_infer._parser()):
        base = ["--input", "i", "--output", "o", "--intrinsics", "k"]
        args = ap.parse_args(base)
        assert args.penetration is False and args.resolve_penetration is False
        args = ap.parse_args(base + ["--penetration", "--resolve-penetration"])
        assert args.penetration and args.resolve_penetration
    assert EP.NEW_KEYS == ("penetration_depth_m", "penetration_mean_m", "penetration_vertices", "contact_vertices", "vertices_signed_distance",
                           "vertices_contact")
    assert EP.RESOLVE_KEYS == ("cam_t_unresolved", "penetration_shift_m", "penetration_resolved")
    for fn in (EP.score_folder, EP.annotate_folder, EP.resolve_folder):
        assert inspect.signature(fn).parameters["contact_tol_m"].default == PN.CONTACT_TOL_M == 0.002


def _hand(rng, cam_t, right):
    return {"betas": rng.normal(0, 0.5, 10).astype(np.float32), "pose_hand": rng.normal(0, 0.1, 45).astype(np.float32),
            "pose_global": rng.normal(0, 0.3, 3).astype(np.float32), "cam_t": np.array(cam_t, np.float32), "is_right": right}


def test_record_fold(tmp_path, monkeypatch):
    """New keys only on two-hand records; every other key keeps its object; one-hand records are copied byte for byte."""
    from hamer_yolo_amd import evaluate_penetration as EP
    rng = np.random.default_rng(5)
    data = {"right": _hand(rng, (0, 0, 0.5), True), "left": _hand(rng, (0.02, 0, 0.5), False), "note": "kept"}
    found = {t: {"codes": np.full(778, k, np.uint8), "signed_distance": np.full(778, -0.001 * (k + 1), np.float32), "max_depth_m": 0.004 + k,
                 "mean_depth_m": 0.002, "inside": 30 + k, "contact": 12, "tested": 400, "status": 0,
                 "shift": np.array([0.001 * (1 - 2 * k), 0.0, -0.002]), "resolved": True} for k, t in enumerate(EP.SIDES)}
    out = EP.annotated_record(data, found)
    assert out["note"] is data["note"] and set(out) == set(data)
    for k, t in enumerate(EP.SIDES):
        h = out[t]
        assert set(h) == set(data[t]) | set(EP.NEW_KEYS) and all(h[key] is data[t][key] for key in data[t])
        assert h["penetration_depth_m"] == 0.004 + k and isinstance(h["penetration_depth_m"], float) and h["penetration_mean_m"] == 0.002
        assert h["penetration_vertices"] == 30 + k and h["contact_vertices"] == 12 and isinstance(h["penetration_vertices"], int)
        assert h["vertices_signed_distance"].dtype == np.float32 and h["vertices_signed_distance"].shape == (778,)
        assert h["vertices_contact"].dtype == np.uint8 and h["vertices_contact"].tolist() == [k] * 778
    out = EP.resolved_record(data, found)
    for k, t in enumerate(EP.SIDES):
        h = out[t]
        assert set(h) == set(data[t]) | set(EP.NEW_KEYS) | set(EP.RESOLVE_KEYS)
        assert all(h[key] is data[t][key] for key in data[t] if key != "cam_t") and h["cam_t_unresolved"] is data[t]["cam_t"]
        assert h["cam_t"].dtype == np.float32 and h["cam_t"].shape == (3,) and h["penetration_resolved"] is True
        assert np.array_equal(h["cam_t"], (data[t]["cam_t"].astype(np.float64) + found[t]["shift"]).astype(np.float32))
        assert h["penetration_shift_m"].dtype == np.float32 and np.allclose(h["penetration_shift_m"], found[t]["shift"])
    # the folder functions on a stubbed scan: one two-hand record, one one-hand record, one without hands
    src, dst = tmp_path / "src", tmp_path / "dst"
    src.mkdir()
    records = {"r0": data, "r1": {"right": _hand(rng, (0, 0, 0.6), True), "left": None}, "r2": {"right": None, "left": None}}
    for stem, rec in records.items():
        np.save(src / f"{stem}.npy", rec)
    jobs = EP._jobs(str(src), 0, 1)
    assert [(j[0], j[3]) for j in jobs] == [("r0", ["right", "left"]), ("r1", ["right"]), ("r2", [])]
    monkeypatch.setattr(EP, "_scan", lambda *a, **k: (jobs, {0: found}))
    assert EP.annotate_folder(str(src), str(dst), None) == {"records": 3, "annotated": 1, "penetrating": 1}
    for stem in ("r1", "r2"):
        assert open(dst / f"{stem}.npy", "rb").read() == open(src / f"{stem}.npy", "rb").read()
    back = np.load(dst / "r0.npy", allow_pickle=True).item()
    assert set(back["right"]) == set(data["right"]) | set(EP.NEW_KEYS) and back["note"] == "kept"
    assert EP.resolve_folder(str(src), str(dst), None) == {"records": 3, "annotated": 1, "moved": 1, "unresolved": 0}
    assert "cam_t_unresolved" in np.load(dst / "r0.npy", allow_pickle=True).item()["left"]
    res = EP.score_folder(str(src), None)
    assert res["two_hand_records"] == 1 and res["penetrating_records"] == 1 and res["max_depth_m"] == 1.004 and len(res["rows"]) == 2
    assert "1 interpenetrate" in EP.format_line(res)
