"""Host checks of the visibility rules (hm_point_visibility, hm_mesh_coverage, hamer.utils.visibility, evaluate_visibility): the
numpy rule of tests/visibility_rule.py against an independent vectorised point test and an independent per-pixel coverage
loop, the two identities, scenes with known answers, the ellipsoid against the analytic facing test, and the surface --
exports, header, build list, argument checks, the Python layer, the drivers' parsers and folds.  No GPU."""
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
import visibility_rule as VR  # noqa: E402
import zrender_rule as ZR  # noqa: E402

from hamer_yolo_amd import build as B  # noqa: E402
from hamer_yolo_amd import lib as L  # noqa: E402
from hamer_yolo_amd.hamer.utils import visibility as V  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K240 = np.array([[600.0, 0.0, 160.0], [0.0, 600.0, 120.0], [0.0, 0.0, 1.0]])


def square(half, z, cx=0.0, cy=0.0, n=8):
    """A fronto-parallel square of side 2 * half at depth z, an (n+1) x (n+1) vertex grid: (vertices, faces)."""
    g = np.linspace(-half, half, n + 1)
    xx, yy = np.meshgrid(g + cx, g + cy)
    v = np.stack([xx.ravel(), yy.ravel(), np.full(xx.size, z)], 1)
    f = []
    for j in range(n):
        for i in range(n):
            a = j * (n + 1) + i
            f += [(a, a + 1, a + n + 2), (a, a + n + 2, a + n + 1)]
    return v, np.asarray(f, np.int32)


def small_scene(seed, H=29, W=37):
    """Two overlapping random fans and a sliver in one small view, with a sensor that has holes and a label image."""
    rng = np.random.default_rng(seed)
    K = np.array([[40.0, 0.3, W / 2.0 + 0.25], [0.0, 42.0, H / 2.0 - 0.5], [0.0, 0.0, 1.0]])
    meshes = []
    for z in (0.5, 0.42, 0.6):
        v = np.concatenate([rng.uniform(-0.25, 0.25, (9, 2)), z + rng.uniform(-0.03, 0.03, (9, 1))], 1)
        f = rng.integers(0, 9, (10, 3)).astype(np.int32)
        meshes.append({"frame": 0, "vertices": v, "faces": f})
    meshes[2]["faces"][0] = (0, 0, 1)                                    # zero area
    meshes[2]["faces"][1] = (0, 1, 12)                                   # a corner index outside the mesh
    f0 = 0
    for m in meshes:
        m["face_id0"], f0 = f0, f0 + len(m["faces"])
    r = ZR.render(1, H, W, K, meshes)
    sensor = DR.sensor_from_depth(r["depth"], 0.001, wall_m=0.8)
    sensor[0, :, : W // 3] = 380                                         # something nearer than every mesh
    sensor[rng.random(sensor.shape) < 0.1] = 0
    mask = rng.choice(np.array([0, 3, 5], np.uint8), (1, H, W), p=[0.2, 0.6, 0.2])
    return K, meshes, r, sensor, mask


# ------------------------------------------------------------------ the rules
def vectorised_codes(depth, mesh_id, K, pts, g, window, znear, sensor, unit, raw_range, scene_tol_m, mask):
    """The point rule again, over all points of one group at once and with the window as shifted maps."""
    N, H, W = mesh_id.shape
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    code = np.full(len(pts), -1, np.int64)
    with np.errstate(all="ignore"):
        behind = ~(z >= znear)
        u = ((K[0, 0] * x + K[0, 1] * y) + K[0, 2] * z) / z
        v = ((K[1, 0] * x + K[1, 1] * y) + K[1, 2] * z) / z
        inside = (np.abs(u) < 65536.0) & (np.abs(v) < 65536.0)
    px = np.where(inside & ~behind, np.floor(np.rint(256.0 * np.where(inside, u, 0)) / 256.0), -1).astype(np.int64)
    py = np.where(inside & ~behind, np.floor(np.rint(256.0 * np.where(inside, v, 0)) / 256.0), -1).astype(np.int64)
    view = g["view"]
    outside = ~((px >= 0) & (px < W) & (py >= 0) & (py < H)) | (not 0 <= view < N)
    code[outside] = VR.OUTSIDE
    code[behind] = VR.BEHIND
    live = np.nonzero(code < 0)[0]
    if len(live) == 0:
        return code
    mid, dep = mesh_id[view], depth[view].astype(np.float64)
    hand = np.zeros(len(live), bool)
    any_valid, clear = np.zeros(len(live), bool), np.zeros(len(live), bool)
    for dy in range(-window, window + 1):
        for dx in range(-window, window + 1):
            xx, yy = px[live] + dx, py[live] + dy
            ok = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
            xc, yc = np.clip(xx, 0, W - 1), np.clip(yy, 0, H - 1)
            cov = mid[yc, xc] >= 0
            hand |= ok & cov & (dep[yc, xc] >= z[live] - g["tol_m"])
            if dx == 0 and dy == 0:
                hand |= ~cov
            if sensor is not None:
                raw = sensor[view][yc, xc].astype(np.int64)
                val = ok & (raw != 0) & (raw >= raw_range[0]) & (raw <= raw_range[1])
                any_valid |= val
                clear |= val & (raw.astype(np.float64) * unit >= z[live] - scene_tol_m)
    centre = mid[py[live], px[live]]
    res = np.where(~hand, np.where(centre == g["mesh"], VR.SELF, VR.OTHER), VR.VISIBLE)
    res = np.where(hand & any_valid & ~clear, VR.SCENE, res)
    lab = g.get("label", -2)
    if mask is not None and lab != -2:
        mv = mask[view][py[live], px[live]]
        passes = mv != 0 if lab == -1 else (mv == lab if 0 <= lab <= 255 else np.zeros(len(live), bool))
        res = np.where((res == VR.VISIBLE) & ~passes, VR.OFF_MASK, res)
    code[live] = res
    return code


@pytest.mark.parametrize("window", [0, 1, 2])
@pytest.mark.parametrize("with_sensor,with_mask", [(False, False), (True, False), (True, True)])
def test_point_rule_against_vectorised_form(window, with_sensor, with_mask):
    K, meshes, r, sensor, mask = small_scene(3)
    rng = np.random.default_rng(window)
    own = np.concatenate([m["vertices"] for m in meshes])
    pts = np.concatenate([own, own + rng.normal(0, 0.01, own.shape), rng.uniform(-0.4, 0.4, (60, 3)) + (0, 0, 0.5),
                          [[0.0, 0.0, 0.04], [np.nan, 0.0, 0.5], [0.0, 0.0, np.nan], [0.0, 0.0, np.inf], [1e6, 0.0, 0.06]]])
    kw = dict(sensor=sensor if with_sensor else None, unit=0.001, raw_range=(100, 700), scene_tol_m=0.01, mask=mask if with_mask else None)
    groups = [dict(view=0, mesh=0, p0=0, np=40, tol_m=0.003, label=-1), dict(view=0, mesh=1, p0=40, np=30, tol_m=0.015, label=3),
              dict(view=0, mesh=2, p0=75, np=len(pts) - 75, tol_m=0.003, label=300), dict(view=4, mesh=0, p0=70, np=5, tol_m=0.003)]
    codes, counts = VR.point_visibility(r["depth"], r["mesh_id"], K, pts, groups, window=window, **kw)
    for gi, g in enumerate(groups):
        sl = slice(g["p0"], g["p0"] + g["np"])
        want = vectorised_codes(r["depth"], r["mesh_id"], K, pts[sl], g, window, 0.05, kw["sensor"], 0.001, (100, 700), 0.01, kw["mask"])
        assert (codes[sl] == want).all(), (gi, np.nonzero(codes[sl] != want)[0][:5])
        assert (counts[gi, :7] == np.bincount(want, minlength=7)).all() and counts[gi, 7] == g["np"]
    assert set(np.unique(codes)) >= {VR.VISIBLE, VR.BEHIND, VR.OUTSIDE}
    assert (codes[70:75] == VR.OUTSIDE).all()                            # the group whose view is outside the batch


def pixel_loop_coverage(mesh, K, H, W, znear=0.05):
    """Per pixel, per face, in Python integers: the coverage rule with no vectorisation and no pixel boxes."""
    fx, _, ok = ZR.project(mesh["vertices"], K, znear)
    cov = np.zeros((H, W), bool)
    nv = len(mesh["vertices"])
    for f in np.asarray(mesh["faces"]).tolist():
        if any(not 0 <= c < nv for c in f) or not all(ok[c] for c in f):
            continue
        (x0, y0), (x1, y1), (x2, y2) = (tuple(int(t) for t in fx[c]) for c in f)
        area = (x1 - x0) * (y2 - y0) - (y1 - y0) * (x2 - x0)
        if area == 0:
            continue
        if area < 0:
            x1, y1, x2, y2 = x2, y2, x1, y1
        edges = (((x1, y1), (x2, y2)), ((x2, y2), (x0, y0)), ((x0, y0), (x1, y1)))
        for py in range(H):
            for px in range(W):
                sx, sy = 256 * px + 128, 256 * py + 128
                inside = True
                for (ax, ay), (bx, by) in edges:
                    e = (bx - ax) * (sy - ay) - (by - ay) * (sx - ax)
                    owns = by - ay < 0 or (by - ay == 0 and bx - ax > 0)
                    inside = inside and (e > 0 or (e == 0 and owns))
                cov[py, px] |= inside
    return cov


@pytest.mark.parametrize("seed", [3, 8])
def test_coverage_against_a_pixel_loop_and_the_identities(seed):
    K, meshes, r, sensor, mask = small_scene(seed)
    H, W = r["mesh_id"].shape[1:]
    labels = [-1, 3, -2]
    counts, boxes = VR.mesh_coverage(H, W, K, meshes, r["depth"], r["mesh_id"], sensor=sensor, unit=0.001, raw_range=(100, 700),
                                     scene_tol_m=0.01, mask=mask, labels=labels)
    for m, mesh in enumerate(meshes):
        cov = pixel_loop_coverage(mesh, K, H, W)
        assert (cov.reshape(-1) == VR.covered_by(mesh, K, H, W)).all()
        mid, dep = r["mesh_id"][0], r["depth"][0].astype(np.float64)
        modal = cov & (mid == m)
        assert counts[m, 0] == cov.sum() and counts[m, 1] == modal.sum() == (mid == m).sum()
        assert counts[m, 2] == (cov & (mid >= 0) & (mid != m)).sum() and counts[m, 7] == 0
        raw = sensor[0].astype(np.int64)
        valid = (raw >= 100) & (raw <= 700)
        scene = modal & valid & (raw * 0.001 < dep - 0.01)
        assert counts[m, 4] == scene.sum() and counts[m, 5] == (modal & ~valid).sum()
        off = {-1: mask[0] == 0, 3: mask[0] != 3, -2: np.zeros_like(cov)}[labels[m]]
        assert counts[m, 6] == (modal & ~scene & off).sum()
        ys, xs = np.nonzero(cov)
        assert boxes[m, :4].tolist() == ([xs.min(), ys.min(), xs.max(), ys.max()] if len(ys) else [-1] * 4)
    assert (counts[:, 0] == counts[:, 1] + counts[:, 2] + counts[:, 7]).all()
    assert (counts[:, 1] == counts[:, 3] + counts[:, 4] + counts[:, 6]).all()
    assert counts[:, 0].min() > 0 and counts[:, 2].max() > 0 and counts[:, 4].max() > 0 and counts[:, 6].max() > 0
    # against maps that are not these meshes' render: uncovered_in_map and the identities
    empty = np.full_like(r["mesh_id"], -1)
    c2, b2 = VR.mesh_coverage(H, W, K, meshes, np.zeros_like(r["depth"]), empty)
    assert (c2[:, 7] == c2[:, 0]).all() and (c2[:, 1:7] == 0).all() and (b2[:, 4:] == -1).all() and (b2[:, :4] == boxes[:, :4]).all()


# ------------------------------------------------------------------ known answers
def _scene(meshes, H=240, W=320, K=K240):
    f0 = 0
    for m in meshes:
        m.setdefault("frame", 0)
        m["face_id0"], f0 = f0, f0 + len(m["faces"])
    return ZR.render(1, H, W, K, meshes)


def _hands(meshes, r, H=240, W=320, K=K240, **kw):
    start = np.cumsum([0] + [len(m["vertices"]) for m in meshes])
    groups = [dict(view=0, mesh=i, p0=int(start[i]), np=len(m["vertices"]), tol_m=0.003) for i, m in enumerate(meshes)]
    codes, cp = VR.point_visibility(r["depth"], r["mesh_id"], K, np.concatenate([m["vertices"] for m in meshes]), groups, window=1, **kw)
    cx, boxes = VR.mesh_coverage(H, W, K, meshes, r["depth"], r["mesh_id"], **kw)
    return [codes[start[i]:start[i + 1]] for i in range(len(meshes))], cp, cx, boxes, VR.summary(cp, cx)


def test_known_answers_two_squares():
    bv, bf = square(0.03, 0.5)
    fv, ff = square(0.04, 0.4)
    meshes = [{"vertices": bv, "faces": bf}, {"vertices": fv, "faces": ff}]
    codes, cp, cx, boxes, s = _hands(meshes, _scene(meshes))
    assert (codes[0] == VR.OTHER).all() and (codes[1] == VR.VISIBLE).all()
    assert cx[0, 1] == 0 and cx[0, 2] == cx[0, 0] > 1000 and s["visible_share"][0] == 0.0 and s["occluded_by_hand"][0] == 1.0
    assert s["visible_share"][1] == 1.0 and cx[1, 3] == cx[1, 1] == cx[1, 0]
    assert boxes[0, 4:].tolist() == [-1] * 4 and boxes[1, :4].tolist() == boxes[1, 4:].tolist()
    assert boxes[0, :4].tolist() == [124, 84, 195, 155]                 # 160 +- 36 px and 120 +- 36 px, centres inside
    assert (s["in_frame"] == 1.0).all()


def test_known_answers_wall():
    v, f = square(0.05, 0.5)
    meshes = [{"vertices": v, "faces": f}]
    r = _scene(meshes)
    sensor = np.full((1, 240, 320), 1000, np.uint16)
    sensor[:, :, :160] = 300                                             # a wall at 0.3 m over the left half of the frame
    codes, cp, cx, boxes, s = _hands(meshes, r, sensor=sensor, unit=0.001, raw_range=(1, 65535), scene_tol_m=0.01)
    modal_left = ((r["mesh_id"][0] == 0)[:, :160]).sum()
    assert cx[0, 4] == modal_left > 0 and cx[0, 3] == cx[0, 1] - modal_left and cx[0, 5] == 0
    u = 600.0 * v[:, 0] / 0.5 + 160.0
    assert (codes[0][u < 158.5] == VR.SCENE).all() and (codes[0][u > 161.5] == VR.VISIBLE).all()
    assert s["occluded_by_scene"][0] == float(modal_left) / float(cx[0, 0])
    sensor[:] = 0                                                        # no valid reading: nothing changes a point or a pixel
    codes, cp, cx, boxes, s = _hands(meshes, r, sensor=sensor, unit=0.001, raw_range=(1, 65535), scene_tol_m=0.01)
    assert (codes[0] == VR.VISIBLE).all() and cx[0, 4] == 0 and cx[0, 5] == cx[0, 1] == cx[0, 3]


def test_known_answers_half_out_of_frame():
    v, f = square(0.05, 0.5, cx=-0.16 * 0.5 / 0.6 * 1.0, n=10)           # centred on u = 160 - 160 = 0: the left border
    meshes = [{"vertices": v, "faces": f}]
    codes, cp, cx, boxes, s = _hands(meshes, _scene(meshes))
    u = 600.0 * v[:, 0] / 0.5 + 160.0
    assert (codes[0][u < -0.5] == VR.OUTSIDE).all() and (codes[0][u > 0.5] == VR.VISIBLE).all()
    n_out = int((codes[0] == VR.OUTSIDE).sum())
    assert n_out == 55 and s["in_frame"][0] == 1.0 - 55.0 / 121.0        # five columns left of the border; the sixth rounds onto X = 0
    assert boxes[0, :4].tolist() == [0, 60, 59, 179] == boxes[0, 4:].tolist()   # clipped at x = 0; 120 +- 60 px
    assert cx[0, 0] == 60 * 120 and s["visible_share"][0] == 1.0


ELLIPSOIDS = [((0.05, 0.08, 0.02), 0.0, (0, 529, 52, 577)), ((0.05, 0.08, 0.02), 0.6, (0, 535, 36, 571)),
              ((0.04, 0.09, 0.03), 1.2, (3, 514, 32, 592))]


@pytest.mark.parametrize("semi,turn,want", ELLIPSOIDS)
def test_ellipsoid_against_the_analytic_facing_test(semi, turn, want):
    """tol_m = 0.003, window = 1, 240 x 320, K = 600 / 600 / 160 / 120, centre (0.01, -0.005, 0.5).  A vertex faces the camera
    when n . p < 0 (n the ellipsoid's normal there, p the vertex in the camera frame)."""
    v, f = DR.ellipsoid(semi)
    c, s = np.cos(turn), np.sin(turn)
    R = np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])
    p = v @ R.T + np.array([0.01, -0.005, 0.5])
    n = (v / np.asarray(semi) ** 2) @ R.T
    facing = (n * p).sum(1) < 0
    meshes = [{"vertices": p, "faces": f}]
    r = _scene(meshes)
    codes, counts = VR.point_visibility(r["depth"], r["mesh_id"], K240, p, [dict(view=0, mesh=0, p0=0, np=len(p), tol_m=0.003)], window=1)
    vis = codes == VR.VISIBLE
    got = (int((facing & ~vis).sum()), int(facing.sum()), int((~facing & vis).sum()), int((~facing).sum()))
    print("facing not VISIBLE %d of %d, back-facing VISIBLE %d of %d" % got)
    assert got[0] <= 0.01 * got[1]
    assert got[2] <= 0.12 * got[3]
    assert got == want                                                  # the numpy prototype's counts, pinned
    assert set(np.unique(codes)) == {VR.VISIBLE, VR.SELF}               # one mesh: what is hidden is hidden by itself
    cx, _ = VR.mesh_coverage(240, 320, K240, meshes, r["depth"], r["mesh_id"])
    assert cx[0, 0] == cx[0, 1] == cx[0, 3] == (r["mesh_id"] == 0).sum()  # front and back faces share pixels: counted once


# ------------------------------------------------------------------ surface
NAMES = ("hm_point_visibility", "hm_mesh_coverage_workspace_bytes", "hm_mesh_coverage")


def test_surface():
    header = open(os.path.join(ROOT, "include", "hamer_hip.h")).read()
    lib = L.load()
    for name in NAMES:
        assert re.search(r"\b%s\(" % name, header) and name in L.EXPORTS and hasattr(lib, name), name
    assert "visibility.hip" in B.SOURCES and os.path.exists(os.path.join(B.CSRC, "visibility.hip"))
    assert "---- Visibility" in header and "an uncovered\n *      neighbour is neutral" in header
    assert int(re.search(r"#define HM_VERSION (\d+)", header).group(1)) == L.HM_VERSION == lib.hm_version() == 402
    src = open(os.path.join(B.CSRC, "visibility.hip")).read()
    assert "#pragma clang fp contract(off)" in src and '#include "raster_tiles.h"' in src
    for word in ("getenv", "hipMalloc", "asm", "hipDeviceSynchronize", "hipStreamSynchronize", "printf"):
        assert word not in src, word
    assert lib.hm_mesh_coverage_workspace_bytes.restype is C.c_size_t
    assert len(lib.hm_point_visibility.argtypes) == 21 and len(lib.hm_mesh_coverage.argtypes) == 25
    assert C.sizeof(L.VisGroup) == 32 and L.VisGroup.view.offset == 8 and L.VisGroup.label.offset == 24
    assert re.search(r"hm_vis_group \{ double tol_m; int32_t view, mesh, p0, np, label, reserved; \}", header)
    assert V.CODES == ("VISIBLE", "BEHIND", "OUTSIDE", "SELF", "OTHER", "SCENE", "OFF_MASK")
    for i, name in enumerate(V.CODES):
        assert re.search(r"HM_VIS_%s = %d\b" % (name, i), header) and getattr(V, name) == getattr(VR, name) == i


def test_workspace_bytes():
    lib = L.load()
    ws = lib.hm_mesh_coverage_workspace_bytes
    assert ws(0, 4, 4, 1, 1, 1) == 0 and ws(1, 4, 4, -1, 1, 1) == 0 and ws(1, 4, 4, 0, 0, 0) > 0
    small, big = ws(1, 1080, 1920, 778 * 4, 4, 1538 * 4), ws(16, 1080, 1920, 778 * 64, 64, 1538 * 64)
    assert small < big < 16 * small + 4096 and small % 256 == 0
    assert ws(64, 1080, 1920, 0, 1, 1) == ws(1, 1080, 1920, 0, 1, 1)      # no per-pixel buffer: N plays no part
    assert big < lib.hm_mesh_render_workspace_bytes(16, 1080, 1920, 778 * 64, 64, 1538 * 64) // 20


K_OK = (C.c_double * 18)(*([600.0, 0.0, 160.0, 0.0, 600.0, 120.0, 0.0, 0.0, 1.0] * 2))
K_BAD = (C.c_double * 18)(*([600.0, 0.0, 160.0, 0.0, 600.0, 120.0, 0.0, 0.0, 1.0] + [600.0, 0.0, 160.0, 0.0, 600.0, 120.0, 0.0, 1e-9, 1.0]))
INF, NAN = float("inf"), float("nan")
P_ORDER = ("depth", "mesh_id", "N", "H", "W", "K", "znear", "points", "P", "groups", "G", "window", "sensor", "unit", "raw_lo", "raw_hi",
           "scene_tol_m", "mask", "codes", "counts", "stream")
C_ORDER = ("N", "H", "W", "K", "verts", "n_verts", "faces", "n_faces", "meshes", "n_meshes", "znear", "depth", "mesh_id", "sensor", "unit",
           "raw_lo", "raw_hi", "scene_tol_m", "mask", "labels", "counts", "boxes", "workspace", "workspace_bytes", "stream")


def _table(frame=0, v0=0, nv=10, f0=0, nf=12):
    t = (L.Mesh * 2)()
    t[0].frame, t[0].v0, t[0].nv, t[0].f0, t[0].nf = frame, v0, nv, f0, nf
    t[1].frame, t[1].v0, t[1].nv, t[1].f0, t[1].nf = 1, 10, 10, 12, 8
    return t


def _points(**kw):
    """hm_point_visibility over MADE-UP device addresses that are never dereferenced: every case must fail in the host part."""
    a = dict(depth=0x10000, mesh_id=0x20000, N=2, H=37, W=53, K=K_OK, znear=0.05, points=0x30000, P=100, groups=0x40000, G=3, window=1,
             sensor=0x50000, unit=0.001, raw_lo=1, raw_hi=65535, scene_tol_m=0.01, mask=0x60000, codes=0x70000, counts=0x80000, stream=None)
    a.update(kw)
    lib = L.load()
    rc = lib.hm_point_visibility(*[a[k] for k in P_ORDER])
    return rc, lib.hm_last_error_string().decode()


def _coverage(**kw):
    a = dict(N=2, H=37, W=53, K=K_OK, verts=0x30000, n_verts=20, faces=0x40000, n_faces=20, meshes=_table(), n_meshes=2, znear=0.05,
             depth=0x10000, mesh_id=0x20000, sensor=0x50000, unit=0.001, raw_lo=1, raw_hi=65535, scene_tol_m=0.01, mask=0x60000,
             labels=0x90000, counts=0x70000, boxes=0x80000, workspace=0xA0000, workspace_bytes=None, stream=None)
    a.update(kw)
    lib = L.load()
    if a["workspace_bytes"] is None:
        a["workspace_bytes"] = int(lib.hm_mesh_coverage_workspace_bytes(2, 37, 53, 20, 2, 20))
    rc = lib.hm_mesh_coverage(*[a[k] for k in C_ORDER])
    return rc, lib.hm_last_error_string().decode()


COMMON_BAD = [
    (dict(depth=None), "null"), (dict(mesh_id=None), "null"), (dict(K=None), "null"), (dict(counts=None), "null"),
    (dict(N=0), "N, H, W"), (dict(H=0), "N, H, W"), (dict(W=-1), "N, H, W"), (dict(N=1024, H=1024, W=2048), "2^31"),
    (dict(znear=0.0), "znear"), (dict(znear=-1.0), "znear"), (dict(znear=INF), "znear"), (dict(znear=NAN), "znear"),
    (dict(unit=0.0), "unit"), (dict(unit=INF), "unit"), (dict(unit=NAN), "unit"), (dict(scene_tol_m=0.0), "scene_tol_m"),
    (dict(scene_tol_m=-0.01), "scene_tol_m"), (dict(scene_tol_m=NAN), "scene_tol_m"), (dict(raw_lo=10, raw_hi=9), "raw_lo"),
    (dict(K=K_BAD), "last row"), (dict(depth=0x10002), "aligned"), (dict(mesh_id=0x20002), "aligned"), (dict(sensor=0x50001), "aligned"),
]


@pytest.mark.parametrize("kw,word", COMMON_BAD + [
    (dict(points=None), "null"), (dict(groups=None), "null"), (dict(codes=None), "null"),
    (dict(window=-1), "window"), (dict(window=3), "window"), (dict(G=-1), "negative"), (dict(P=-1), "negative"),
    (dict(points=0x30004), "aligned"), (dict(groups=0x40004), "aligned"), (dict(counts=0x80002), "aligned"),
])
def test_point_visibility_argument_checks(kw, word):
    rc, msg = _points(**kw)
    assert rc == -1 and "hm_point_visibility" in msg and word in msg, (rc, msg)          # HM_ERR_ARG


@pytest.mark.parametrize("kw,word", COMMON_BAD + [
    (dict(verts=None), "null"), (dict(faces=None), "null"), (dict(meshes=None), "null"), (dict(boxes=None), "null"),
    (dict(workspace=None), "null"), (dict(n_meshes=-1), "negative"), (dict(n_verts=-1), "negative"), (dict(n_faces=-1), "negative"),
    (dict(H=32768, W=2, N=1), "32767"), (dict(workspace_bytes=0), "workspace too small"), (dict(workspace_bytes=1000), "workspace too small"),
    (dict(verts=0x30004), "aligned"), (dict(counts=0x70004), "aligned"), (dict(workspace=0xA0004), "aligned"),
    (dict(faces=0x40002), "aligned"), (dict(boxes=0x80002), "aligned"), (dict(labels=0x90002), "aligned"),
    (dict(meshes=_table(frame=2)), "view outside"), (dict(meshes=_table(nv=11)), "share vertices"), (dict(meshes=_table(nf=13)), "share faces"),
    (dict(meshes=_table(v0=-1)), "negative mesh range"), (dict(n_verts=19), "outside the vertex or face array"),
])
def test_mesh_coverage_argument_checks(kw, word):
    rc, msg = _coverage(**kw)
    assert rc == -1 and "hm_mesh_coverage" in msg and word in msg, (rc, msg)             # HM_ERR_ARG


def test_nothing_to_do_passes_the_checks_without_a_launch():
    assert _points(G=0)[0] == 0 and _points(G=0, points=None, groups=None, codes=None, counts=None, sensor=None, mask=None, P=0)[0] == 0
    assert _coverage(n_meshes=0)[0] == 0
    assert _coverage(n_meshes=0, verts=None, faces=None, meshes=None, counts=None, boxes=None, workspace=None, workspace_bytes=0,
                     n_verts=0, n_faces=0, sensor=None, mask=None, labels=None)[0] == 0
    assert _points(G=0, sensor=None, unit=0.0, scene_tol_m=NAN, raw_lo=5, raw_hi=1)[0] == 0   # read only with a sensor


# ------------------------------------------------------------------ the Python layer
def test_python_layer_raises_without_a_gpu_and_on_bad_inputs():
    d, i = torch.zeros(1, 4, 5), torch.zeros(1, 4, 5, dtype=torch.int32)
    pts = torch.zeros(3, 3, dtype=torch.float64)
    with pytest.raises(ValueError, match="GPU"):
        V.point_visibility(d, i, np.eye(3), pts, [dict(view=0, mesh=0, p0=0, np=3, tol_m=0.003)])
    with pytest.raises(ValueError, match="GPU"):
        V.mesh_coverage(4, 5, np.eye(3), [], d, i)
    with pytest.raises(ValueError):
        V.point_visibility(d.numpy(), i.numpy(), np.eye(3), pts, [])
    with pytest.raises(ValueError, match="no hands"):
        V.hand_visibility(4, 5, np.eye(3), [], torch.zeros(0, 21, 3))
    p = inspect.signature(V.point_visibility).parameters
    assert list(p)[:5] == ["depth", "mesh_id", "K", "points", "groups"]
    assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(p)[5:])
    assert [p[k].default for k in ("window", "znear", "sensor", "unit", "raw_range", "scene_tol_m", "mask")] == \
        [1, 0.05, None, 0.001, (1, 65535), 0.01, None]
    p = inspect.signature(V.mesh_coverage).parameters
    assert list(p)[:6] == ["H", "W", "K", "meshes", "depth", "mesh_id"] and {"sensor", "mask", "labels"} <= set(p)
    p = inspect.signature(V.hand_visibility).parameters
    assert list(p)[:5] == ["H", "W", "K", "meshes", "joints"]
    assert (p["vertex_tol_m"].default, p["joint_tol_m"].default, p["window"].default) == (0.003, 0.015, 1)
    for fn in (V.hand_visibility, V):
        assert "choices, not measurements" in " ".join(fn.__doc__.split())
    assert V._ws == {} and V.release_workspaces() is None
    raw = V.pack_groups([dict(view=1, mesh=2, p0=3, np=4, tol_m=0.25, label=-1), dict(view=5, mesh=6, p0=7, np=8, tol_m=0.5)])
    assert raw.dtype == np.uint8 and raw.size == 64
    assert raw[:8].view(np.float64)[0] == 0.25 and raw[8:32].view(np.int32).tolist() == [1, 2, 3, 4, -1, 0]
    assert raw[40:64].view(np.int32).tolist() == [5, 6, 7, 8, -2, 0]


def test_summary_matches_the_rule_and_handles_empty_rows():
    cp = np.array([[700, 10, 40, 20, 5, 2, 1, 778], [0, 0, 0, 0, 0, 0, 0, 0], [0, 0, 778, 0, 0, 0, 0, 778]])
    cx = np.array([[1000, 800, 150, 700, 60, 5, 40, 50], [0] * 8, [0] * 8])
    s, w = V.summary(cp, cx), VR.summary(cp, cx)
    for k in ("visible_share", "occluded_by_hand", "occluded_by_scene", "in_frame"):
        assert s[k].dtype == np.float64 and np.array_equal(s[k], w[k], equal_nan=True), k
    assert s["visible_share"][0] == 0.7 and s["occluded_by_hand"][0] == 0.15 and s["occluded_by_scene"][0] == 0.06
    assert s["in_frame"][0] == 1.0 - 50.0 / 778.0 and np.isnan(s["visible_share"][1:]).all()
    assert np.isnan(s["in_frame"][1]) and s["in_frame"][2] == 0.0
    both = np.stack([cp, cp[::-1]], 1)                                  # (n, 2, 8): the vertex rows are taken
    assert np.array_equal(V.summary(both, cx)["in_frame"], s["in_frame"], equal_nan=True)


# ------------------------------------------------------------------ the drivers: parsers, folds, fallbacks
def test_driver_parsers_and_defaults():
    from hamer_yolo_amd import d_infer, infer
    from hamer_yolo_amd import evaluate_visibility as EV
    a = EV._parser().parse_args(["--pred", "A", "--intrinsics", "K.txt"])
    assert (a.depth_maps, a.unit, a.masks, a.label, a.images, a.write_to) == (None, 0.001, None, 3, None, None)
    a = EV._parser().parse_args(["--pred", "A", "--intrinsics", "K", "--depth-maps", "D", "--unit", "0.0001", "--masks", "M", "--label", "5",
                                 "--images", "I", "--write-to", "O"])
    assert (a.depth_maps, a.unit, a.masks, a.label, a.images, a.write_to) == ("D", 0.0001, "M", 5, "I", "O")
    for bad in (["--pred", "A"], ["--intrinsics", "K"]):
        with pytest.raises(SystemExit):
            EV._parser().parse_args(bad)
    for bad in (["--unit", "0.01"], ["--label", "4"], [], ["--images", "I", "--unit", "0"]):       # usage errors before any model is loaded
        with pytest.raises(SystemExit) as e:
            EV.main(["--pred", "A", "--intrinsics", "K"] + bad)
        assert e.value.code == 2
    p = inspect.signature(EV.score_folder).parameters
    assert list(p)[:3] == ["npy_folder", "hamer", "k_real"] and p["depth_folder"].default is None and p["mask_folder"].default is None
    assert (p["unit"].default, p["label"].default, p["rank"].default, p["world"].default) == (0.001, 3, 0, 1)
    p = inspect.signature(EV.annotate_folder).parameters
    assert list(p)[:4] == ["npy_folder", "out_folder", "hamer", "k_real"]
    with pytest.raises(ValueError, match="frame size"):
        EV.score_folder("A", None, np.eye(3))
    with pytest.raises(ValueError, match="label"):
        EV.score_folder("A", None, np.eye(3), image_folder="I", label=0)
    assert EV.NEW_KEYS == ("joints_visible", "vertices_visible", "visible_share", "in_frame", "amodal_box", "modal_box", "visibility_counts")
    a = infer._parser().parse_args(["--input", "A", "--output", "B"])
    assert a.visibility is False and a.visible_joints is False
    a = infer._parser().parse_args(["--input", "A", "--output", "B", "--visibility", "--render", "R", "--render-keypoints", "over", "--visible-joints"])
    assert a.visibility is True and a.visible_joints is True
    assert infer.render_keypoint_args(infer._parser(), a)["visible_joints"] is True
    plain = infer._parser().parse_args(["--input", "A", "--output", "B", "--render", "R", "--render-keypoints", "over"])
    assert "visible_joints" not in infer.render_keypoint_args(infer._parser(), plain)      # the default calls render_folder as before
    a = d_infer._parser().parse_args(["--input", "A", "--output", "B", "--intrinsics", "K", "--visibility"])
    assert a.visibility is True and d_infer._parser().parse_args(["--input", "A", "--output", "B", "--intrinsics", "K"]).visibility is False
    for bad in (["--visible-joints"], ["--render", "R", "--visible-joints"]):
        with pytest.raises(SystemExit) as e:
            infer.main(["--input", "A", "--output", "B"] + bad)
        assert e.value.code == 2
    src = inspect.getsource(infer)
    assert src.index("def _mask_fit_args") < src.index("def _visibility_args") < src.index("def mask_args")
    assert src.index("refine_records(args, hamer, rank, world)") < src.index("visibility_records(args, hamer, rank, world")


def _hand(seed):
    rng = np.random.default_rng(seed)
    return {"betas": rng.normal(size=10).astype(np.float32), "pose_hand": rng.normal(size=45).astype(np.float32),
            "pose_global": rng.normal(size=3).astype(np.float32), "cam_t": np.array([0.0, 0.0, 0.6], np.float32), "is_right": True}


def test_annotate_fold_and_a_record_without_hands(tmp_path, monkeypatch):
    from hamer_yolo_amd import evaluate_visibility as EV
    rec = {"right": _hand(1), "left": None}
    found = {"right": {"joints": np.arange(21) % 7, "vertices": np.arange(778) % 5, "boxes": np.array([1, 2, 30, 40, -1, -1, -1, -1]),
                       "pixels": np.arange(8), "visible_share": 0.25, "in_frame": float("nan")}}
    out = EV.annotated_record(rec, found)
    assert out["left"] is None and out is not rec and set(out["right"]) == set(rec["right"]) | set(EV.NEW_KEYS)
    assert all(out["right"][k] is rec["right"][k] for k in rec["right"]) and "joints_visible" not in rec["right"]
    h = out["right"]
    assert h["joints_visible"].dtype == np.uint8 and h["joints_visible"].tolist() == (np.arange(21) % 7).tolist()
    assert h["vertices_visible"].dtype == np.uint8 and h["vertices_visible"].shape == (778,)
    assert h["amodal_box"].dtype == np.int32 and h["amodal_box"].tolist() == [1, 2, 30, 40] and h["modal_box"].tolist() == [-1] * 4
    assert h["visibility_counts"].dtype == np.int64 and h["visibility_counts"].tolist() == list(range(8))
    assert h["visible_share"] == 0.25 and np.isnan(h["in_frame"])
    assert EV.annotated_record(rec, {}) == rec and EV.annotated_record({"right": None, "left": None}, found) == {"right": None, "left": None}
    # a folder whose only records have no hands, or no frame: nothing is rendered (no GPU is touched), the files are copied
    import types
    npy, img, dst = tmp_path / "npy", tmp_path / "img", tmp_path / "dst"
    npy.mkdir(); img.mkdir()
    np.save(npy / "e0.npy", {"right": None, "left": None})
    np.save(npy / "e1.npy", rec)                                         # a hand, but no frame to take the size from
    from PIL import Image
    Image.fromarray(np.zeros((8, 8, 3), np.uint8)).save(img / "e0.png")
    hamer = types.SimpleNamespace(device=torch.device("cpu"), mano=types.SimpleNamespace(faces=np.zeros((1, 3), np.int32)), cfg=None)
    r = EV.annotate_folder(str(npy), str(dst), hamer, np.eye(3), image_folder=str(img))
    assert r == {"records": 2, "hands": 1, "annotated": 0, "skipped": ["e1"], "n_skipped": 1}
    for f in ("e0.npy", "e1.npy"):
        assert open(dst / f, "rb").read() == open(npy / f, "rb").read()
    s = EV.score_folder(str(npy), hamer, np.eye(3), image_folder=str(img))
    assert s["rows"] == [] and s["hands"] == 0 and s["skipped"] == ["e1"] and all(np.isnan(v) for v in s["means"].values())
    assert "0 hands" in EV.format_line(s)


def test_render_folder_fallback_and_joint_confidences(capsys):
    from hamer_yolo_amd import render
    flags = np.zeros(21, np.uint8)
    flags[[3, 8]], flags[20] = 4, 2
    render._said_no_flags.clear()
    conf = render.joint_confidences([{"joints_visible": flags}, {"cam_t": 0}, {"joints_visible": np.full(21, 3)}, {}])
    assert conf.dtype == np.float32 and conf.shape == (4, 21)
    assert conf[0].tolist() == [0.0 if j in (3, 8, 20) else 1.0 for j in range(21)]
    assert (conf[1] == 1).all() and (conf[2] == 0).all() and (conf[3] == 1).all()
    said = capsys.readouterr().out
    assert said.count("joints_visible") >= 1 and said.count("\n") == 1   # a record without the key draws all joints: said once
    p = inspect.signature(render.render_folder).parameters
    assert p["visible_joints"].default is False and list(p)[-1] == "visible_joints"
    with pytest.raises(ValueError, match="visible_joints"):
        render.render_folder("A", "B", "C", None, visible_joints=True)
