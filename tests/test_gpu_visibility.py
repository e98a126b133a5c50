"""GPU checks of the visibility kernels (hm_point_visibility, hm_mesh_coverage; hamer.utils.visibility) and of the drivers
that stand on them.  Every comparison of codes, counts and boxes is exact equality with the numpy rule of
tests/visibility_rule.py; the cross-check against the renderer's own maps uses no rule file at all."""
import ctypes as C
import os
import sys
import time

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import depth_eval_rule as DR  # noqa: E402
import visibility_rule as VR  # noqa: E402
import zrender_rule as ZR  # noqa: E402

from hamer_yolo_amd import lib as L  # noqa: E402
from hamer_yolo_amd import render  # noqa: E402
from hamer_yolo_amd.hamer.utils import visibility as V  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
SENSOR = dict(unit=0.001, raw_range=(100, 700), scene_tol_m=0.01)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def gpu_meshes(meshes):
    """On the device; faces_checked: the scenes hold corner indices outside their mesh on purpose (the kernels skip such faces)."""
    return [{"frame": m["frame"], "vertices": dev(np.asarray(m["vertices"], np.float64)), "faces": dev(np.asarray(m["faces"], np.int32)),
             "faces_checked": True} for m in meshes]


def camera(H, W):
    """Powers of two and whole numbers: a point built from a pixel position projects back onto it exactly."""
    return np.array([[64.0, 0.0, float(W // 2)], [0.0, 64.0, float(H // 2)], [0.0, 0.0, 1.0]])


def at_pixel(K, u, v, z):
    return [(u - K[0, 2]) * z / K[0, 0], (v - K[1, 2]) * z / K[1, 1], z]


def fan(rng, cx, cy, z, r=0.2, nv=9, nf=10):
    v = np.concatenate([rng.uniform(-r, r, (nv, 2)) + (cx, cy), z + rng.uniform(-0.03, 0.03, (nv, 1))], 1)
    return v, rng.integers(0, nv, (nf, 3)).astype(np.int32)


def maps_of(N, H, W, K, meshes):
    """The GPU's own render of the meshes, on the device and on the host."""
    r = render.render_views(H, W, K, gpu_meshes(meshes), outputs=("depth", "mesh_id"), views=N, device=DEV)
    return r["depth"], r["mesh_id"], r["depth"].cpu().numpy(), r["mesh_id"].cpu().numpy()


def side_maps(rng, N, H, W, depth_h):
    sensor = DR.sensor_from_depth(depth_h, 0.001, wall_m=0.65)
    sensor[:, :, : W // 3] = 380                                         # nearer than every mesh
    sensor[:, : H // 4, :] = 900                                         # outside raw_range: no measurement
    sensor[rng.random(sensor.shape) < 0.1] = 0
    mask = rng.choice(np.array([0, 3, 5], np.uint8), (N, H, W), p=[0.2, 0.6, 0.2])
    return sensor, mask


# ------------------------------------------------------------------ a: point visibility
def point_scene(H, W):
    rng = np.random.default_rng(H * 1000 + W)
    K = camera(H, W)
    ext = (W / 128.0 * 0.5, H / 128.0 * 0.5)                             # half the view's extent at z = 0.5
    meshes = [{"frame": n, "vertices": v, "faces": f} for n, z in ((0, 0.5), (0, 0.44), (1, 0.5), (1, 0.56))
              for v, f in [fan(rng, rng.uniform(-0.3, 0.3) * ext[0], rng.uniform(-0.3, 0.3) * ext[1], z, r=0.8 * max(ext))]]
    z = 0.5
    us = [0.5, 1.5, 2.5, W / 2.0, W - 2.5, W - 1.5, W - 0.5]
    vs = [0.5, 1.5, H / 2.0, H - 1.5, H - 0.5] if H > 3 else [0.5, 1.5, 2.5]
    grid = [at_pixel(K, u, v, zz) for u in us for v in vs for zz in (0.3, 0.5, 0.7)]                      # every border and corner
    edges = [at_pixel(K, float(u), float(v), z) for u in (0, 1, W // 2, W - 1, W) for v in (0, 1, H - 1, H)]   # X a multiple of 256
    special = [at_pixel(K, -1.0 / 256, 1.5, z), at_pixel(K, -1.0 / 512, 1.5, z), at_pixel(K, -3.0 / 512, 1.5, z),
               at_pixel(K, 1.5, -1.0 / 256, z), at_pixel(K, 65536.0 - 1.0 / 256, 1.5, z), at_pixel(K, 65536.0, 1.5, z),
               at_pixel(K, -65536.0, 1.5, z), at_pixel(K, 1.5, 65536.0, z), [0.0, 0.0, np.nan], [np.nan, 0.0, 0.5], [0.0, 0.0, np.inf],
               [0.0, 0.0, -np.inf], [0.0, 0.0, np.nextafter(0.05, 0.0)], [0.0, 0.0, 0.05], [0.0, 0.0, 0.0], [0.0, 0.0, -0.5]]
    own = np.concatenate([m["vertices"] for m in meshes])
    near = np.concatenate([own, own + rng.normal(0, 0.004, own.shape), own + (0, 0, 0.02), own - (0, 0, 0.02)])
    many = np.concatenate([rng.uniform(-ext[0], ext[0], (1000, 1)) * 1.1, rng.uniform(-ext[1], ext[1], (1000, 1)) * 1.1,
                           rng.uniform(0.03, 0.7, (1000, 1))], 1)
    parts = [np.asarray(grid), np.asarray(edges), np.asarray(special), near, many]
    start = np.cumsum([0] + [len(p) for p in parts])
    g = lambda view, mesh, part, tol, label, lo=0, hi=None: dict(                                          # noqa: E731
        view=view, mesh=mesh, p0=int(start[part]) + lo, np=(len(parts[part]) if hi is None else hi) - lo, tol_m=tol, label=label)
    groups = [g(0, 0, 0, 0.003, -2), g(0, 1, 1, 0.003, -1), g(0, 0, 2, 0.015, 3),                          # three groups on view 0
              g(1, 2, 3, 0.003, 300, 0, 60), g(1, 3, 3, 0.015, 3, 60, 130),                                # two on view 1
              g(1, 2, 3, 0.003, -1, 130, 130),                                                             # np == 0
              g(5, 0, 3, 0.003, -2, 130, 136), g(-1, 0, 3, 0.003, 3, 136, 140),                            # views outside the batch
              g(0, 1, 4, 0.003, 3)]                                                                        # 1000 points: several workgroups
    return K, meshes, np.concatenate(parts), groups


@pytest.mark.parametrize("H,W", [(40, 70), (3, 64)])
def test_point_visibility_shapes(H, W):
    K, meshes, pts, groups = point_scene(H, W)
    depth, mesh_id, depth_h, mid_h = maps_of(2, H, W, K, meshes)
    assert (mid_h >= 0).any() and (mid_h < 0).any()
    sensor, mask = side_maps(np.random.default_rng(5), 2, H, W, depth_h)
    seen = set()
    for window in (0, 1, 2):
        for with_sensor, with_mask in ((False, False), (True, False), (False, True), (True, True)):
            kw = dict(SENSOR, sensor=sensor if with_sensor else None, mask=mask if with_mask else None)
            want_codes, want_counts = VR.point_visibility(depth_h, mid_h, K, pts, groups, window=window, **kw)
            kw.update(sensor=dev(sensor) if with_sensor else None, mask=dev(mask) if with_mask else None)
            codes, counts = V.point_visibility(depth, mesh_id, K, dev(pts), groups, window=window, **kw)
            codes, counts = codes.cpu().numpy(), counts.cpu().numpy()
            bad = np.nonzero(codes != want_codes)[0]
            assert len(bad) == 0, (window, with_sensor, with_mask, bad[:8], codes[bad[:8]], want_codes[bad[:8]], pts[bad[:8]])
            assert np.array_equal(counts, want_counts) and counts.dtype == np.int32
            assert (counts[:, :7].sum(1) == counts[:, 7]).all() and counts[5].tolist() == [0] * 8
            seen |= set(np.unique(codes).tolist())
    assert seen == {0, 1, 2, 3, 4, 5, 6, 255}                            # every code, and points in no group untouched


# ------------------------------------------------------------------ b: coverage
def coverage_scene(H, W):
    rng = np.random.default_rng(H + W)
    K = camera(H, W)
    ex, ey = W / 128.0 * 0.5, H / 128.0 * 0.5
    meshes = []
    for n, (cx, cy) in enumerate([(-ex, 0.0), (ex, 0.0), (0.0, -ey), (0.0, ey)]):                          # across each border
        v, f = fan(rng, cx, cy, 0.5, r=0.5 * max(ex, ey))
        meshes.append({"frame": n % 2, "vertices": v, "faces": f})
    v, f = fan(rng, 5 * ex, 0.0, 0.5, r=0.1)
    meshes.append({"frame": 0, "vertices": v, "faces": f})                                                  # wholly outside
    v, f = fan(rng, 0.0, 0.0, 0.02, r=0.01)
    meshes.append({"frame": 1, "vertices": v, "faces": f})                                                  # wholly behind znear
    v, f = fan(rng, 0.0, 0.0, 0.48, r=0.6 * max(ex, ey), nf=14)
    f[0], f[1], f[2], f[3] = (0, 0, 1), (2, 3, 2), (0, 1, 9), (-1, 2, 3)                                    # zero area, bad corner indices
    v[4] = v[5]                                                                                            # zero area by position
    f[4] = (4, 5, 6)
    meshes.append({"frame": 0, "vertices": v, "faces": f})
    ev, ef = DR.ellipsoid((0.3 * ex, 0.5 * ey, 0.05), n_lat=8, n_lon=12)                                   # closed: front and back share pixels
    meshes.append({"frame": 1, "vertices": ev + (0.1 * ex, 0.0, 0.45), "faces": ef})
    meshes.append({"frame": 1, "vertices": ev * (1.5, 0.6, 1.0) + (0.3 * ex, 0.1 * ey, 0.52), "faces": ef})   # overlaps it, behind
    corner = np.array([at_pixel(K, 16.0, 16.0, 0.5), at_pixel(K, 32.0, 17.0, 0.5), at_pixel(K, 16.5, 32.0, 0.5), at_pixel(K, 3.0, 3.0, 0.5)])
    meshes.append({"frame": 0, "vertices": corner, "faces": np.array([[0, 1, 2], [0, 2, 3]], np.int32)})    # a corner on a tile corner
    return K, meshes


def box_of(sel):
    ys, xs = np.nonzero(sel)
    return [int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max())] if len(ys) else [-1] * 4


def check_against_the_renderer(counts, boxes, mid_h, meshes):
    """No rule file: a mesh's modal pixels are the pixels the renderer labelled with it."""
    for m, mesh in enumerate(meshes):
        own = mid_h[mesh["frame"]] == m
        assert counts[m, 1] == own.sum() and counts[m, 7] == 0 and boxes[m, 4:].tolist() == box_of(own), m
    assert (counts[:, 0] == counts[:, 1] + counts[:, 2] + counts[:, 7]).all()
    assert (counts[:, 1] == counts[:, 3] + counts[:, 4] + counts[:, 6]).all()


@pytest.mark.parametrize("H,W", [(40, 70), (33, 130)])
def test_coverage_shapes(H, W):
    K, meshes = coverage_scene(H, W)
    depth, mesh_id, depth_h, mid_h = maps_of(2, H, W, K, meshes)
    sensor, mask = side_maps(np.random.default_rng(9), 2, H, W, depth_h)
    labels = [(-2, -1, 3, 300, 5)[m % 5] for m in range(len(meshes))]
    gm = gpu_meshes(meshes)
    for with_sensor, with_mask in ((False, False), (True, False), (False, True), (True, True)):
        kw = dict(SENSOR, sensor=sensor if with_sensor else None, mask=mask if with_mask else None, labels=labels if with_mask else None)
        want_counts, want_boxes = VR.mesh_coverage(H, W, K, meshes, depth_h, mid_h, **kw)
        kw.update(sensor=dev(sensor) if with_sensor else None, mask=dev(mask) if with_mask else None,
                  labels=dev(np.asarray(labels, np.int32)) if with_mask else None)     # a tensor: 300 is no label the host check lets by
        counts, boxes = V.mesh_coverage(H, W, K, gm, depth, mesh_id, **kw)
        counts, boxes = counts.cpu().numpy(), boxes.cpu().numpy()
        assert np.array_equal(counts, want_counts), (with_sensor, with_mask, counts, want_counts)
        assert np.array_equal(boxes, want_boxes) and counts.dtype == np.int64 and boxes.dtype == np.int32
        check_against_the_renderer(counts, boxes, mid_h, meshes)
    assert (counts[[4, 5]] == 0).all() and (boxes[[4, 5]] == -1).all()    # outside, behind: nothing anywhere
    assert counts[8, 2] > 0 and counts[7, 0] == counts[7, 1] > 0         # the ellipsoid behind the other one; the front one whole
    assert counts[:, 4].max() > 0 and counts[:, 5].max() > 0 and counts[:, 6].max() > 0
    assert (boxes[:4, 0].min(), boxes[:4, 1].min(), boxes[:4, 2].max(), boxes[:4, 3].max()) == (0, 0, W - 1, H - 1)
    V.release_workspaces(); render.release_workspaces()


def test_fifty_one_face_meshes():
    """More meshes than one setup launch takes (48)."""
    H, W = 40, 70
    K = camera(H, W)
    rng = np.random.default_rng(50)
    meshes = []
    for i in range(50):
        c = rng.uniform(-1.0, 1.0, 2) * (0.2, 0.1)
        tri = np.array([[-0.08, -0.07], [0.08, -0.05], [0.0, 0.08]]) * (1.0 if i % 2 else -1.0)          # both windings
        v = np.concatenate([c + tri + rng.uniform(-0.02, 0.02, (3, 2)), rng.uniform(0.4, 0.6, (3, 1))], 1)
        meshes.append({"frame": i % 3, "vertices": v, "faces": np.array([[0, 1, 2]], np.int32)})
    depth, mesh_id, depth_h, mid_h = maps_of(3, H, W, K, meshes)
    counts, boxes = V.mesh_coverage(H, W, K, gpu_meshes(meshes), depth, mesh_id)
    counts, boxes = counts.cpu().numpy(), boxes.cpu().numpy()
    want_counts, want_boxes = VR.mesh_coverage(H, W, K, meshes, depth_h, mid_h)
    assert np.array_equal(counts, want_counts) and np.array_equal(boxes, want_boxes)
    check_against_the_renderer(counts, boxes, mid_h, meshes)
    assert counts[:, 0].min() > 0 and counts[:, 2].max() > 0 and (counts[:, 1] == 0).any()
    V.release_workspaces(); render.release_workspaces()


def test_large_face_and_shared_edge():
    """Both integer widths of the shared sample test, in the renderer and in the coverage kernel: a triangle whose corner box
    spans more than 2^15 sub-pixel units (the int64 edge functions) behind a square of two small triangles (int32) whose
    common edge runs exactly through pixel centres, and the same two triangles as two meshes of a second view: every pixel on
    the diagonal belongs to exactly one of them."""
    H, W = 24, 40
    K = camera(H, W)
    big = np.array([at_pixel(K, -150.0, -10.0, 0.5), at_pixel(K, 200.0, 5.0, 0.5), at_pixel(K, 20.0, 300.0, 0.5)])
    square = np.array([at_pixel(K, u, v, 0.4) for u, v in ((4.5, 4.5), (20.5, 4.5), (20.5, 20.5), (4.5, 20.5))])
    meshes = [{"frame": 0, "vertices": big, "faces": np.array([[0, 1, 2]], np.int32)},
              {"frame": 0, "vertices": square, "faces": np.array([[0, 1, 2], [0, 2, 3]], np.int32)},
              {"frame": 1, "vertices": square, "faces": np.array([[0, 1, 2]], np.int32)},
              {"frame": 1, "vertices": square, "faces": np.array([[2, 0, 3]], np.int32)}]
    spans = []
    for m in meshes:
        corners, _, _, _, valid = ZR.face_table(m["vertices"], m["faces"], K, 0.05)
        assert valid.all()
        spans += [int((c.max(0) - c.min(0)).max()) for c in corners]
    assert spans[0] >= 32768 and max(spans[1:]) < 32768               # whatever the code under test does, both widths are asked for
    oracle, f0 = [], 0
    for m in meshes:
        oracle.append(dict(m, face_id0=f0))
        f0 += len(m["faces"])
    want = ZR.render(2, H, W, K, oracle)
    depth, mesh_id, depth_h, mid_h = maps_of(2, H, W, K, meshes)
    assert np.array_equal(mid_h, want["mesh_id"]) and np.array_equal(depth_h.view(np.uint32), want["depth"].view(np.uint32))
    assert [int((mid_h[0] == m).sum()) for m in (0, 1)] == [704, 256] and (mid_h[0] >= 0).all()
    assert [int((mid_h[1] == m).sum()) for m in (-1, 2, 3)] == [704, 136, 120]
    counts, boxes = V.mesh_coverage(H, W, K, gpu_meshes(meshes), depth, mesh_id)
    counts, boxes = counts.cpu().numpy(), boxes.cpu().numpy()
    want_counts, want_boxes = VR.mesh_coverage(H, W, K, meshes, want["depth"], want["mesh_id"])
    assert np.array_equal(counts, want_counts) and np.array_equal(boxes, want_boxes)
    check_against_the_renderer(counts, boxes, mid_h, meshes)
    assert counts[:, 0].tolist() == [960, 256, 136, 120]
    assert boxes[:, 4:].tolist() == [[0, 0, 39, 23], [4, 4, 19, 19], [4, 4, 19, 19], [4, 5, 18, 19]]
    V.release_workspaces(); render.release_workspaces()


# ------------------------------------------------------------------ c: batch invariance, buffers
def test_batch_invariance_in_bytes():
    H, W = 40, 70
    K, meshes = coverage_scene(H, W)
    one = dict(meshes[7], frame=0)                                        # the closed ellipsoid, alone in its view
    sensor, mask = side_maps(np.random.default_rng(2), 3, H, W, np.zeros((3, H, W), np.float32))
    pts = np.concatenate([one["vertices"], one["vertices"] + (0, 0, 0.03)])
    g = dict(view=0, mesh=0, p0=0, np=len(pts), tol_m=0.003, label=3)

    def alone():
        depth, mesh_id, _, _ = maps_of(1, H, W, K, [one])
        kw = dict(SENSOR, sensor=dev(sensor[1:2]), mask=dev(mask[1:2]))
        codes, cp = V.point_visibility(depth, mesh_id, K, dev(pts), [g], window=1, **kw)
        cx, bx = V.mesh_coverage(H, W, K, gpu_meshes([one]), depth, mesh_id, labels=[3], **kw)
        return [t.cpu().numpy().tobytes() for t in (codes, cp, cx, bx)]

    def inside():
        batch = [dict(meshes[0], frame=0), dict(meshes[8], frame=2), dict(one, frame=1), dict(meshes[6], frame=0)]
        depth, mesh_id, _, _ = maps_of(3, H, W, K, batch)
        kw = dict(SENSOR, sensor=dev(sensor), mask=dev(mask))
        filler = np.random.default_rng(1).uniform(-0.3, 0.3, (333, 3)) + (0, 0, 0.5)
        allp = np.concatenate([filler, pts, filler[:77]])
        groups = [dict(view=0, mesh=0, p0=0, np=333, tol_m=0.01, label=-1), dict(view=2, mesh=1, p0=333 + len(pts), np=77, tol_m=0.003, label=-2),
                  dict(g, view=1, mesh=2, p0=333)]
        codes, cp = V.point_visibility(depth, mesh_id, K, dev(allp), groups, window=1, **kw)
        cx, bx = V.mesh_coverage(H, W, K, gpu_meshes(batch), depth, mesh_id, labels=[-1, -2, 3, 5], **kw)
        cp = cp[2].cpu().numpy().copy()
        return [codes[333:333 + len(pts)].cpu().numpy().tobytes(), cp.tobytes(), cx[2].cpu().numpy().tobytes(), bx[2].cpu().numpy().tobytes()]

    a, b = alone(), inside()
    assert a == b and alone() == a and inside() == b
    assert np.frombuffer(a[2], np.int64)[0] > 100
    V.release_workspaces(); render.release_workspaces()


def test_buffers_have_canaries_and_points_in_no_group_are_untouched():
    H, W = 40, 70
    K, meshes, pts, groups = point_scene(H, W)
    depth, mesh_id, depth_h, mid_h = maps_of(2, H, W, K, meshes)
    lib = L.load()
    Kh = np.ascontiguousarray(np.broadcast_to(K, (2, 3, 3)))
    P, G, pad = len(pts), len(groups), 64
    codes = torch.full((P + 2 * pad,), 0xA5, dtype=torch.uint8, device=DEV)
    counts = torch.full((G * 8 + 2 * pad,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    gd, pd = dev(V.pack_groups(groups)), dev(pts)
    L.check(lib.hm_point_visibility(L.ptr(depth), L.ptr(mesh_id), 2, H, W, Kh.ctypes.data_as(C.POINTER(C.c_double)), 0.05, L.ptr(pd), P,
                                    L.ptr(gd), G, 1, None, 0.0, 0, 0, 0.0, None, codes.data_ptr() + pad, counts.data_ptr() + 4 * pad,
                                    L.current_stream()), "hm_point_visibility")
    want_codes, want_counts = VR.point_visibility(depth_h, mid_h, K, pts, groups, window=1, codes=np.full(P, 0xA5, np.uint8))
    codes, counts = codes.cpu().numpy(), counts.cpu().numpy()
    assert (codes[:pad] == 0xA5).all() and (codes[-pad:] == 0xA5).all() and np.array_equal(codes[pad:-pad], want_codes)
    assert (want_codes == 0xA5).sum() > 0                                # the gaps between the groups
    assert (counts[:pad] == 0x5A5A5A5A).all() and (counts[-pad:] == 0x5A5A5A5A).all()
    assert np.array_equal(counts[pad:-pad].reshape(G, 8), want_counts)
    # coverage: canaries round counts and boxes, a workspace of exactly the size asked for
    K2, cm = coverage_scene(H, W)
    depth, mesh_id, depth_h, mid_h = maps_of(2, H, W, K2, cm)
    table, vd, fd, v0, f0 = render._pack_meshes(gpu_meshes(cm), DEV, 2)
    n = len(cm)
    need = int(lib.hm_mesh_coverage_workspace_bytes(2, H, W, v0, n, f0))
    ws = torch.full((need + 2 * 256,), 0xA5, dtype=torch.uint8, device=DEV)
    cnt = torch.full((n * 8 + 2 * pad,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=DEV)
    box = torch.full((n * 8 + 2 * pad,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    for _ in range(2):                                                    # the second call finds the first one's results in place
        L.check(lib.hm_mesh_coverage(2, H, W, Kh.ctypes.data_as(C.POINTER(C.c_double)), L.ptr(vd), v0, L.ptr(fd), f0, table, n, 0.05,
                                     L.ptr(depth), L.ptr(mesh_id), None, 0.0, 0, 0, 0.0, None, None, cnt.data_ptr() + 8 * pad,
                                     box.data_ptr() + 4 * pad, ws.data_ptr() + 256, need, L.current_stream()), "hm_mesh_coverage")
    want_counts, want_boxes = VR.mesh_coverage(H, W, K2, cm, depth_h, mid_h)
    cnt, box, ws = cnt.cpu().numpy(), box.cpu().numpy(), ws.cpu().numpy()
    assert (cnt[:pad] == 0x5A5A5A5A5A5A5A5A).all() and (cnt[-pad:] == 0x5A5A5A5A5A5A5A5A).all()
    assert (box[:pad] == 0x5A5A5A5A).all() and (box[-pad:] == 0x5A5A5A5A).all()
    assert (ws[:256] == 0xA5).all() and (ws[-256:] == 0xA5).all()
    assert np.array_equal(cnt[pad:-pad].reshape(n, 8), want_counts) and np.array_equal(box[pad:-pad].reshape(n, 8), want_boxes)
    render.release_workspaces()


# ------------------------------------------------------------------ d: hand_visibility
def two_hands():
    """Two closed ellipsoids in one view, the second half hidden behind the first, and 21 'joints' inside each."""
    H, W = 120, 160
    K = np.array([[300.0, 0.0, 80.0], [0.0, 300.0, 60.0], [0.0, 0.0, 1.0]])
    ev, ef = DR.ellipsoid((0.04, 0.07, 0.02), n_lat=12, n_lon=24)
    placed = [ev + (-0.02, 0.0, 0.5), ev + (0.02, 0.01, 0.58)]
    meshes = [{"frame": 0, "vertices": p, "faces": ef} for p in placed]
    joints = np.stack([0.7 * ev[::13][:21] + c for c in ((-0.02, 0.0, 0.5), (0.02, 0.01, 0.58))])
    return H, W, K, meshes, joints


def test_hand_visibility_equals_the_rule_and_does_not_wait(monkeypatch):
    H, W, K, meshes, joints = two_hands()
    gm = gpu_meshes(meshes)
    got = V.hand_visibility(H, W, K, gm, dev(joints))                     # warm: modules loaded, workspaces cached
    torch.cuda.synchronize()
    mid_h, depth_h = got["mesh_id"].cpu().numpy(), got["depth"].cpu().numpy()
    nv = len(meshes[0]["vertices"])
    groups = [dict(view=0, mesh=i, p0=p0, np=n, tol_m=tol) for i in (0, 1) for p0, n, tol in ((i * nv, nv, 0.003), (2 * nv + 21 * i, 21, 0.015))]
    pts = np.concatenate([meshes[0]["vertices"], meshes[1]["vertices"], joints.reshape(-1, 3)])
    want_codes, want_counts = VR.point_visibility(depth_h, mid_h, K, pts, groups, window=1)
    want_cx, want_boxes = VR.mesh_coverage(H, W, K, meshes, depth_h, mid_h)
    assert np.array_equal(got["vertex_codes"].cpu().numpy(), want_codes[:2 * nv]) and got["vertex_start"].tolist() == [0, nv, 2 * nv]
    assert np.array_equal(got["joint_codes"].cpu().numpy(), want_codes[2 * nv:].reshape(2, 21))
    assert np.array_equal(got["counts_points"].cpu().numpy(), want_counts.reshape(2, 2, 8))
    assert np.array_equal(got["counts_pixels"].cpu().numpy(), want_cx) and np.array_equal(got["boxes"].cpu().numpy(), want_boxes)
    s = V.summary(got["counts_points"], got["counts_pixels"])
    assert s["visible_share"][0] == 1.0 and 0.2 < s["visible_share"][1] < 0.8 and s["occluded_by_hand"][0] == 0.0
    assert want_cx[1, 2] + want_cx[1, 3] == want_cx[1, 0] and s["occluded_by_hand"][1] > 0.2 and (s["in_frame"] == 1.0).all()
    assert want_counts[2, VR.OTHER] > 0 and want_counts[3, VR.OTHER] > 0 and want_counts[0, VR.OTHER] == 0
    # half a second of earlier work on the stream is still running when hand_visibility returns
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    torch.cuda._sleep(1000000)
    t1.record()
    torch.cuda.synchronize()
    spin = int(1000000 * 500.0 / max(t0.elapsed_time(t1), 1e-3))
    jd = dev(joints)
    torch.cuda.synchronize()
    torch.cuda._sleep(spin)
    busy = torch.cuda.Event()
    busy.record()
    start = time.perf_counter()
    again = V.hand_visibility(H, W, K, [dict(m, faces_checked=True) for m in gm], jd)
    waited = busy.query()
    print("hand_visibility enqueued in %.1f ms" % ((time.perf_counter() - start) * 1e3))
    assert not waited
    assert all(torch.equal(again[k], got[k]) for k in ("vertex_codes", "joint_codes", "counts_points", "counts_pixels", "boxes"))
    V.release_workspaces(); render.release_workspaces()


# ------------------------------------------------------------------ e: the drivers, on a synthetic MANO model
class _Cfg:
    ckpt_path = "synthetic:0"
    model_cfg = None
    use_onnx = False
    onnx_path = None


FH, FW = 192, 256
FK = np.array([[300.0, 0.0, 128.0], [0.0, 300.0, 96.0], [0.0, 0.0, 1.0]], np.float32)


def same(a, b):
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    if isinstance(a, float) and np.isnan(a):
        return isinstance(b, float) and np.isnan(b)
    return type(a) is type(b) and a == b


def test_drivers_on_a_synthetic_folder(tmp_path, monkeypatch):
    """The folder of test_gpu_depth_eval / test_gpu_mask_driver with one hand placed behind the other (b2), a frame without a
    depth map (b3) and a record without hands (b4)."""
    import json
    from PIL import Image
    from hamer_yolo_amd import evaluate_visibility as EV
    from hamer_yolo_amd import infer
    hi = infer.hamer_inference(_Cfg)
    monkeypatch.setattr(infer, "hamer_inference", lambda cfg: hi)
    npy_dir, img_dir, depth_dir, out_dir, draw_dir = (tmp_path / d for d in ("npy", "img", "depth", "out", "draw"))
    for d in (npy_dir, img_dir, depth_dir):
        d.mkdir()
    np.savetxt(tmp_path / "K.txt", FK)
    rng = np.random.default_rng(33)
    place = {"b0": {"right": (-0.1, 0.0, 0.7)}, "b1": {"left": (0.1, 0.0, 0.7)}, "b2": {"right": (0.0, 0.0, 0.6), "left": (0.04, 0.01, 0.75)},
             "b3": {"right": (0.0, 0.0, 0.7)}, "b4": {}}
    faces = torch.as_tensor(np.asarray(hi.mano.faces, np.int32), device=DEV)
    for stem, sides in place.items():
        Image.fromarray(np.zeros((FH, FW, 3), np.uint8)).save(img_dir / f"{stem}.png")
        rec = {"right": None, "left": None}
        for t, cam_t in sides.items():
            pg, ph = rng.normal(0, 0.3, 3).astype(np.float32), rng.normal(0, 0.15, 45).astype(np.float32)
            rec[t] = {"betas": rng.normal(0, 0.5, 10).astype(np.float32), "theta": np.concatenate([pg, ph]), "pose_hand": ph,
                      "pose_global": pg, "cam_t": np.array(cam_t, np.float32), "is_right": t == "right"}
        np.save(npy_dir / f"{stem}.npy", rec)
        if stem in ("b3", "b4"):
            continue
        hands = [rec[t] for t in ("right", "left") if rec[t] is not None]
        verts = render.camera_vertices(hi, hands)
        meshes = [{"frame": 0, "vertices": verts[j], "faces": faces} for j in range(len(hands))]
        depth = render.render_views(FH, FW, FK, meshes, outputs=("depth",), views=1, device=DEV)["depth"][0].cpu().numpy()
        sensor = DR.sensor_from_depth(depth, 0.001, wall_m=1.5)
        if stem == "b0":
            sensor[:, :100] = 400                                       # a wall in front of the left part of the frame
        np.save(depth_dir / f"{stem}.npy", sensor)
    res = EV.main(["--pred", str(npy_dir), "--intrinsics", str(tmp_path / "K.txt"), "--depth-maps", str(depth_dir), "--images", str(img_dir),
                   "--write-to", str(out_dir), "--json", str(tmp_path / "out.json")])
    assert [(r["stem"], r["hand"]) for r in res["rows"]] == [("b0", "right"), ("b1", "left"), ("b2", "right"), ("b2", "left")]
    assert res["skipped"] == ["b3"] and res["hands"] == 4 and V._ws == {}
    assert res["annotate"] == {"records": 5, "hands": 5, "annotated": 4, "skipped": ["b3"], "n_skipped": 1}
    assert json.load(open(tmp_path / "out.json"))["rows"][3]["pixel_counts"] == res["rows"][3]["pixel_counts"]
    rows = {(r["stem"], r["hand"]): r for r in res["rows"]}
    for r in res["rows"]:
        c = r["pixel_counts"]
        assert c[0] == c[1] + c[2] + c[7] and c[1] == c[3] + c[4] + c[6] and c[7] == 0 and c[0] > 300
        assert sum(r["vertex_counts"][:7]) == r["vertex_counts"][7] == 778 and sum(r["joint_counts"][:7]) == r["joint_counts"][7] == 21
        print(r["stem"], r["hand"], {k: round(r[k], 4) for k in EV.SHARES}, r["joints_visible"], c)
    assert rows[("b2", "left")]["occluded_by_hand"] > 0.2 and rows[("b2", "right")]["occluded_by_hand"] == 0.0
    assert rows[("b2", "left")]["vertex_counts"][VR.OTHER] > 50 and rows[("b2", "left")]["joints_visible"] < 21
    assert rows[("b1", "left")]["visible_share"] == 1.0 and rows[("b1", "left")]["occluded_by_scene"] == 0.0
    assert rows[("b0", "right")]["occluded_by_scene"] > 0.1 and rows[("b0", "right")]["vertex_counts"][VR.SCENE] > 20
    assert abs(res["means"]["visible_share"] - np.mean([r["visible_share"] for r in res["rows"]])) < 1e-15
    # the records: new keys, dtypes and shapes; everything else keeps its bytes; b3 and b4 are copied
    for stem, sides in place.items():
        raw_a, raw_b = (open(d / f"{stem}.npy", "rb").read() for d in (out_dir, npy_dir))
        if stem in ("b3", "b4"):
            assert raw_a == raw_b
            continue
        a, b = (np.load(d / f"{stem}.npy", allow_pickle=True).item() for d in (out_dir, npy_dir))
        for t in ("right", "left"):
            assert (a[t] is None) == (t not in sides)
        for t in sides:
            h = a[t]
            assert set(h) == set(b[t]) | set(EV.NEW_KEYS) and all(same(h[k], b[t][k]) for k in b[t])
            assert h["joints_visible"].dtype == np.uint8 and h["joints_visible"].shape == (21,) and h["joints_visible"].max() <= 6
            assert h["vertices_visible"].dtype == np.uint8 and h["vertices_visible"].shape == (778,)
            assert isinstance(h["visible_share"], float) and isinstance(h["in_frame"], float)
            assert h["amodal_box"].dtype == np.int32 and h["amodal_box"].shape == (4,) and h["modal_box"].shape == (4,)
            assert h["visibility_counts"].dtype == np.int64 and h["visibility_counts"].tolist() == rows[(stem, t)]["pixel_counts"]
            assert h["visible_share"] == rows[(stem, t)]["visible_share"] and h["amodal_box"].tolist() == rows[(stem, t)]["amodal_box"]
            assert np.bincount(h["vertices_visible"], minlength=7).tolist() == rows[(stem, t)]["vertex_counts"][:7]
    # the record's flags are hand_visibility's for the same meshes
    b2 = np.load(out_dir / "b2.npy", allow_pickle=True).item()
    joints, verts = render.camera_joints_vertices(hi, [b2["right"], b2["left"]])
    direct = V.hand_visibility(FH, FW, FK.astype(np.float64), [{"frame": 0, "vertices": verts[j], "faces": faces} for j in (0, 1)], joints,
                               sensor=dev(np.load(depth_dir / "b2.npy")[None]))
    assert np.array_equal(direct["joint_codes"].cpu().numpy(), np.stack([b2["right"]["joints_visible"], b2["left"]["joints_visible"]]))
    assert np.array_equal(direct["vertex_codes"].cpu().numpy(), np.concatenate([b2["right"]["vertices_visible"], b2["left"]["vertices_visible"]]))
    # render_folder(visible_joints=True) draws what skeleton_frames draws with the 0 / 1 confidences
    n = render.render_folder(str(img_dir), str(out_dir), str(draw_dir), hi, FK, keypoints="only", visible_joints=True, ext=".png")
    assert n == 4
    conf = torch.from_numpy(render.joint_confidences([b2["right"], b2["left"]])).to(DEV)
    assert float(conf[1].sum()) < 21 and float(conf[0].sum()) > 0
    kp = torch.cat([render.project_points(joints, FK), conf[..., None]], dim=2)
    want = render.skeleton_frames(torch.zeros(1, FH, FW, 3, dtype=torch.uint8, device=DEV), kp, [0, 0], style="hamer")[0].cpu().numpy()
    got = np.asarray(Image.open(draw_dir / "b2.png"))[:, :, ::-1]
    assert np.array_equal(got, want)
    every = render.skeleton_frames(torch.zeros(1, FH, FW, 3, dtype=torch.uint8, device=DEV), kp[:, :, :2].contiguous(), [0, 0], style="hamer")
    assert not np.array_equal(got, every[0].cpu().numpy())              # the hidden joints and their bones are absent
    render.release_workspaces()


def test_infer_visibility_rewrites_in_place_and_is_off_by_default(tmp_path, monkeypatch):
    """On the precise route a hand's bytes do not depend on the run: without --visibility the files equal those of the Python
    call the --masks line has always made; with it every hand gains the keys and keeps the bytes of the others."""
    from PIL import Image
    from hamer_yolo_amd import evaluate_visibility as EV
    from hamer_yolo_amd import infer, synth
    hi = infer.hamer_inference(_Cfg, precise=True)
    rgb, masks = tmp_path / "rgb", tmp_path / "masks"
    rgb.mkdir(); masks.mkdir()
    for i in range(2):
        Image.fromarray(synth.frame_u8(240, 320, seed=70 + i).numpy()[:, :, ::-1]).save(rgb / f"g{i}.png")
        m = np.zeros((240, 320), np.uint8)
        m[60 + 10 * i:150, 90:170 + 10 * i] = 3
        np.save(masks / f"g{i}.npy", m)
    monkeypatch.setattr(infer, "hamer_inference", lambda cfg: hi)
    outs = [str(tmp_path / d) for d in ("call", "plain", "vis")]
    infer.process_batch_manopara_with_mask(str(rgb), str(masks), outs[0], None, hamer=hi, batched=True, left_label=None, rank=0, world=1,
                                           right_label=3)
    infer.main(["--input", str(rgb), "--output", outs[1], "--masks", str(masks)])
    infer.main(["--input", str(rgb), "--output", outs[2], "--masks", str(masks), "--visibility"])
    for f in ("g0.npy", "g1.npy"):
        raw = [open(os.path.join(o, f), "rb").read() for o in outs]
        assert raw[0] == raw[1] != raw[2]
        a, b = (np.load(os.path.join(o, f), allow_pickle=True).item()["right"] for o in (outs[2], outs[1]))
        assert set(a) == set(b) | set(EV.NEW_KEYS) and all(same(a[k], b[k]) for k in b)
        assert a["joints_visible"].shape == (21,) and a["vertices_visible"].shape == (778,) and a["visibility_counts"].shape == (8,)
        c = a["visibility_counts"]
        assert c[0] == c[1] + c[2] + c[7] and c[1] == c[3] + c[4] + c[6]
    render.release_workspaces()
