"""CPU: the z-buffered renderer's rule (tests/zrender_rule.py, the numpy statement of hm_mesh_render), the argument checks
of its C ABI, the drivers' options and the Python interface that needs no GPU.  The rule tests exercise the numpy
statement alone: they pin the oracle the GPU tests compare against (and state what the rule gives that render_rule.overlay does
not), so they do not depend on the library; the ABI, option and Python tests do."""
import ctypes as C
import inspect

import numpy as np
import pytest

import render_rule as RR
import zrender_rule as ZR
from hamer_yolo_amd import lib as L

HM_ERR_ARG = -1
EYE = np.eye(3)                                      # u = x / z, v = y / z: with z = 1 a vertex (x, y) is the sample (x, y)


S = 5                                                # grid pitch: a jitter of one pixel per vertex keeps every cell's orientation


def _grid_scene(rng, n, flip):
    """An n x n grid of vertices ON pixel centres (k + 0.5, jittered by whole pixels), two triangles per cell, each wound at
    random when `flip`: every edge and every vertex of the mesh lies on sample points."""
    gx, gy = np.meshgrid(np.arange(n + 1) * S, np.arange(n + 1) * S)
    jx, jy = rng.integers(-1, 2, gx.shape), rng.integers(-1, 2, gy.shape)
    jx[[0, -1], :] = 0; jx[:, [0, -1]] = 0; jy[[0, -1], :] = 0; jy[:, [0, -1]] = 0      # a straight outline
    v = np.stack([gx + jx + 0.5, gy + jy + 0.5, np.ones(gx.shape)], -1).reshape(-1, 3)
    idx = np.arange((n + 1) * (n + 1)).reshape(n + 1, n + 1)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[:-1, 1:].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel()
    f = np.concatenate([np.stack([a, b, c], 1), np.stack([b, d, c], 1)])
    if flip:
        sw = rng.random(len(f)) < 0.5
        f[sw] = f[sw][:, [0, 2, 1]]
    return v, f


@pytest.mark.parametrize("flip", [False, True])
def test_watertight_grid_every_interior_sample_exactly_once(flip):
    rng = np.random.default_rng(3 + flip)
    n = 8
    v, f = _grid_scene(rng, n, flip)
    H = W = S * n + 4
    corners, rr, fc, area, valid = ZR.face_table(v, f, EYE, 0.05)
    assert valid.all()
    fi, pix, _ = ZR.cover_pairs(corners, H, W)
    count = np.bincount(pix, minlength=H * W).reshape(H, W)
    # the mesh spans samples 0.5 .. S n + 0.5, i.e. pixels 0 .. S n: all but the trailing row and column exactly once
    assert (count[:S * n, :S * n] == 1).all()
    assert (count[S * n:, :] == 0).all() and (count[:, S * n:] == 0).all()
    for m in (False, True):                              # and the two windings of one mesh cover the same samples
        g = f[:, [0, 2, 1]] if m else f
        c2 = ZR.face_table(v, g, EYE, 0.05)[0]
        assert np.array_equal(np.sort(ZR.cover_pairs(c2, H, W)[1]), np.sort(pix))


def test_interpenetrating_triangles_split_along_their_intersection_line():
    """Two triangles over the same pixels, each a plane whose 1/z is affine in the image: 1/z = 1 + b (u - 20) with b = 0.004
    and b = -0.004.  They cross on the image line u = 20.  Per pixel the nearer one wins, so the region is split along that
    line; the painter's rule of render_rule.overlay gives the whole overlap to one face."""
    H = W = 40
    K = np.array([[1.0, 0, 0], [0, 1.0, 0], [0, 0, 1]])
    meshes = []
    for k, b in enumerate((0.004, -0.004)):
        px = np.array([[2.0, 2.0], [38.0, 3.0], [20.0, 38.0]])
        z = 1.0 / (1.0 + b * (px[:, 0] - 20.0))
        meshes.append({"frame": 0, "vertices": np.concatenate([px * z[:, None], z[:, None]], 1), "faces": np.array([[0, 1, 2]]),
                       "face_id0": k})
    r = ZR.render(1, H, W, K, meshes)
    face = r["face"][0]
    ys, xs = np.nonzero(face >= 0)
    assert len(xs) > 300
    u = xs + 0.5
    # 1/z = 1 + b (u - 20): mesh 0 (b > 0) is nearer where u > 20, mesh 1 where u < 20; u == 20 is no pixel centre
    assert np.array_equal(face[ys, xs], np.where(u > 20.0, 0, 1))
    assert (face == 0).sum() > 100 and (face == 1).sum() > 100
    # the painter's rule hands the whole region to one face
    frames = np.zeros((1, H, W, 3), np.uint8)
    flat = RR.overlay(frames, K, [dict(m, color=(10 + k, 0, 0)) for k, m in enumerate(meshes)], alpha=1.0)[0]
    inner = (face >= 0) & (flat[..., 0] > 0)
    assert len(np.unique(flat[inner][:, 0])) == 1


def test_depth_of_a_fronto_parallel_plane_is_exactly_z():
    z = 0.7317
    px = np.array([[1.3, 2.1], [30.7, 4.9], [12.2, 33.3]])
    m = {"frame": 0, "vertices": np.concatenate([px * z, np.full((3, 1), z)], 1), "faces": np.array([[0, 2, 1]])}
    r = ZR.render(1, 36, 36, EYE, [m])
    cov = r["face"][0] >= 0
    assert cov.sum() > 200
    assert (r["depth"][0][cov] == np.float32(z)).all() and (r["depth"][0][~cov] == 0).all()
    assert (r["rgba"][0][cov][:, 3] == 255).all() and (r["rgba"][0][~cov] == 0).all()
    assert (r["mesh_id"][0][cov] == 0).all() and (r["mesh_id"][0][~cov] == -1).all()


def test_depth_of_a_slanted_plane_matches_the_analytic_depth():
    """Plane n . p = c through the three vertices; along the ray of sample (u, v), z = c / (n . (u, v, 1)).  The rule
    interpolates 1/z between the ROUNDED fixed-point corners, so the samples are taken with corners already on the 1/256
    grid: then the only difference is rounding, a few ulp of fp64 and one of fp32."""
    px = np.array([[2.0, 3.5], [45.25, 6.0], [20.5, 44.75]])               # multiples of 1/256
    z = np.array([0.5, 0.9, 0.65])
    P = np.concatenate([px * z[:, None], z[:, None]], 1)
    r = ZR.render(1, 48, 48, EYE, [{"frame": 0, "vertices": P, "faces": np.array([[0, 1, 2]])}])
    n = np.cross(P[1] - P[0], P[2] - P[0])
    c = n @ P[0]
    ys, xs = np.nonzero(r["face"][0] >= 0)
    assert len(xs) > 300
    want = c / (n[0] * (xs + 0.5) + n[1] * (ys + 0.5) + n[2])
    corners, rr, fc, area, valid = ZR.face_table(P, np.array([[0, 1, 2]]), EYE, 0.05)
    E, hit = ZR.edge_values(np.repeat(corners, len(xs), 0), 256 * xs + 128, 256 * ys + 128)
    assert hit.all()
    A = area[0].astype(np.float64)
    q = (E[0] / A * rr[0, 0] + E[1] / A * rr[0, 1]) + E[2] / A * rr[0, 2]
    assert np.abs(1.0 / q - want).max() <= 1e-12 * np.abs(want).max()
    assert np.array_equal(r["depth"][0][ys, xs], (1.0 / q).astype(np.float32))


def test_vertex_normals_are_summed_in_face_row_order():
    rng = np.random.default_rng(0)
    v = rng.normal(size=(30, 3)) * np.array([1.0, 1e3, 1e-3])              # terms of very different size: the order shows
    f = rng.integers(0, 30, (200, 3))
    f[5] = (31, 0, 1); f[6] = (-1, 2, 3)                                     # invalid rows contribute nothing
    f[7] = (4, 4, 9)                                                         # names vertex 4 twice: once per face
    got = ZR.vertex_normals(v, f)
    want = np.zeros_like(v)
    for row in f:
        if (row < 0).any() or (row >= 30).any():
            continue
        a, c = v[row[1]] - v[row[0]], v[row[2]] - v[row[0]]
        t = np.array([a[1] * c[2] - a[2] * c[1], a[2] * c[0] - a[0] * c[2], a[0] * c[1] - a[1] * c[0]])
        for k in set(row.tolist()):
            want[k] = want[k] + t
    assert np.array_equal(got, want)
    rev = np.zeros_like(v)                                                   # and the order matters for these numbers
    for row in f[::-1]:
        if (row < 0).any() or (row >= 30).any():
            continue
        a, c = v[row[1]] - v[row[0]], v[row[2]] - v[row[0]]
        t = np.array([a[1] * c[2] - a[2] * c[1], a[2] * c[0] - a[0] * c[2], a[0] * c[1] - a[1] * c[0]])
        for k in set(row.tolist()):
            rev[k] = rev[k] + t
    assert not np.array_equal(rev, want)


def test_skipped_faces_and_shading_of_a_facing_plane():
    z = 1.0
    tri = np.array([[2.0, 2.0], [30.0, 3.0], [10.0, 28.0]])
    def mesh(zz):
        return {"frame": 0, "vertices": np.concatenate([tri * np.asarray(zz)[:, None], np.asarray(zz, float)[:, None]], 1),
                "faces": np.array([[0, 1, 2]])}
    assert (ZR.render(1, 32, 32, EYE, [mesh([z, z, z])])["face"] >= 0).any()
    assert not (ZR.render(1, 32, 32, EYE, [mesh([z, z, 0.04])])["face"] >= 0).any()          # one corner nearer than znear
    assert (ZR.render(1, 32, 32, EYE, [mesh([z, z, 0.04])], znear=0.01)["face"] >= 0).any()
    far = mesh([z, z, z]); far["vertices"][1, 0] = 70000.0                                   # |u| >= 2^16
    assert not (ZR.render(1, 32, 32, EYE, [far])["face"] >= 0).any()
    bad = mesh([z, z, z]); bad["faces"] = np.array([[0, 1, 3]])
    assert not (ZR.render(1, 32, 32, EYE, [bad])["face"] >= 0).any()
    flat = mesh([z, z, z]); flat["vertices"][2] = flat["vertices"][1]                       # area 0
    assert not (ZR.render(1, 32, 32, EYE, [flat])["face"] >= 0).any()
    r = ZR.render(1, 32, 32, EYE, [mesh([z, z, z])], base_rgb=(1.0, 0.5, 0.9), bg_rgba=(1, 2, 3, 4),
                  frames=np.full((1, 32, 32, 3), 7, np.uint8))
    cov = r["face"][0] >= 0
    assert (r["rgba"][0][cov] == (255, 128, 230, 255)).all()               # |n.z| = 1: I = 1; rint(127.5) = 128 (half to even)
    assert (r["rgba"][0][~cov] == (1, 2, 3, 4)).all()
    assert (r["out"][0][cov] == (230, 128, 255)).all() and (r["out"][0][~cov] == 7).all()


# ------------------------------------------------------------------ C ABI
def test_render_abi_rejects_bad_arguments_without_gpu():
    lib = L.load()
    assert "hm_mesh_render" in L.EXPORTS and "hm_mesh_render_workspace_bytes" in L.EXPORTS
    assert hasattr(lib, "hm_mesh_render") and hasattr(lib, "hm_mesh_render_workspace_bytes")
    assert L.HM_VERSION == 402 and lib.hm_version() == 402
    ws = lib.hm_mesh_render_workspace_bytes(2, 64, 64, 20, 2, 40)
    assert ws >= 2 * 64 * 64 * 8 + 20 * 24 and lib.hm_mesh_render_workspace_bytes(0, 64, 64, 20, 2, 40) == 0
    P = 1 << 20                                       # fake device addresses: every call below fails before any launch
    meshes = (L.Mesh * 2)()
    meshes[0].frame, meshes[0].v0, meshes[0].nv, meshes[0].f0, meshes[0].nf = 0, 0, 10, 0, 20
    meshes[1].frame, meshes[1].v0, meshes[1].nv, meshes[1].f0, meshes[1].nf = 1, 10, 10, 20, 20
    Kok = np.ascontiguousarray(np.stack([np.array([[500.0, 0, 32], [0, 500.0, 32], [0, 0, 1]])] * 2))

    def kp(K):
        return None if K is None else K.ctypes.data_as(C.POINTER(C.c_double))

    def call(**kw):
        a = dict(N=2, H=64, W=64, K=Kok, verts=P, nv=20, faces=P, nf=40, meshes=meshes, nm=2, base=None, bg=None, znear=0.05,
                 frames=None, out=None, rgba=P * 8, depth=P * 16, mesh_id=P * 32, ws=P * 128, wsb=ws)
        a.update(kw)
        return lib.hm_mesh_render(a["N"], a["H"], a["W"], kp(a["K"]), a["verts"], a["nv"], a["faces"], a["nf"], a["meshes"], a["nm"],
                                  a["base"], a["bg"], a["znear"], a["frames"], a["out"], a["rgba"], a["depth"], a["mesh_id"],
                                  a["ws"], a["wsb"], None)

    assert call(K=None) == HM_ERR_ARG and b"null" in lib.hm_last_error_string()
    assert call(ws=None) == HM_ERR_ARG and b"null" in lib.hm_last_error_string()
    assert call(verts=None) == HM_ERR_ARG and call(faces=None) == HM_ERR_ARG and call(meshes=None) == HM_ERR_ARG
    for row in ((0, 0, 1.0000001), (1e-9, 0, 1), (0, 0.5, 1), (0, 0, np.nan)):
        Kbad = Kok.copy(); Kbad[1, 2] = row
        assert call(K=Kbad) == HM_ERR_ARG and b"last row" in lib.hm_last_error_string()
    for zn in (0.0, -0.05, float("nan"), float("inf")):
        assert call(znear=zn) == HM_ERR_ARG and b"znear" in lib.hm_last_error_string()
    assert call(rgba=None, depth=None, mesh_id=None) == HM_ERR_ARG and b"no output" in lib.hm_last_error_string()
    assert call(frames=P * 64) == HM_ERR_ARG and b"both or neither" in lib.hm_last_error_string()
    assert call(out=P * 64) == HM_ERR_ARG and b"both or neither" in lib.hm_last_error_string()
    assert call(frames=P * 64, out=P * 64 + 5) == HM_ERR_ARG and b"in place" in lib.hm_last_error_string()
    assert call(wsb=ws - 1) == HM_ERR_ARG and b"workspace" in lib.hm_last_error_string()
    assert call(ws=P * 128 + 4) == HM_ERR_ARG and b"8-byte" in lib.hm_last_error_string()
    assert call(depth=P * 16 + 2) == HM_ERR_ARG and b"4-byte" in lib.hm_last_error_string()
    assert call(rgba=P * 8 + 1) == HM_ERR_ARG and call(mesh_id=P * 32 + 3) == HM_ERR_ARG and call(verts=P + 4) == HM_ERR_ARG
    assert call(base=(C.c_double * 3)(1.0, 1.5, 0.9)) == HM_ERR_ARG and b"base_rgb" in lib.hm_last_error_string()
    assert call(nf=39) == HM_ERR_ARG
    meshes[1].f0 = 10
    assert call() == HM_ERR_ARG and b"share faces" in lib.hm_last_error_string()
    meshes[1].f0, meshes[1].v0 = 20, 5
    assert call() == HM_ERR_ARG and b"share vertices" in lib.hm_last_error_string()
    meshes[1].v0, meshes[1].frame = 10, 2
    assert call() == HM_ERR_ARG and b"view" in lib.hm_last_error_string()


def test_header_declares_the_entry_points_and_keeps_the_version():
    import os
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hamer_hip.h")).read()
    assert "int hm_mesh_render(int N, int H, int W, const double* K_host" in hdr
    assert "size_t hm_mesh_render_workspace_bytes(" in hdr
    assert "#define HM_VERSION 402" in hdr


# ------------------------------------------------------------------ drivers and Python
def test_drivers_accept_the_new_options():
    from hamer_yolo_amd import d_infer, infer
    for parser, extra in ((infer._parser, []), (d_infer._parser, ["--intrinsics", "k"])):
        base = ["--input", "i", "--output", "o"] + extra
        a = parser().parse_args(base)
        assert a.hand_maps is None and a.hand_label == 3 and a.render_style == "flat"          # off unless asked for
        a = parser().parse_args(base + ["--render", "r", "--render-style", "smooth", "--hand-maps", "m", "--hand-label", "5"])
        assert a.render_style == "smooth" and a.hand_maps == "m" and a.hand_label == 5
        with pytest.raises(SystemExit):
            parser().parse_args(base + ["--render-style", "pbr"])


def test_mesh_renderer_signature_and_side_view_matrix():
    from hamer_yolo_amd.hamer.utils import mesh_renderer as MR
    with pytest.raises(TypeError):
        MR.MeshRenderer(None)                                               # faces are required
    sig = inspect.signature(MR.MeshRenderer.__call__)
    assert list(sig.parameters) == ["self", "vertices", "camera_translation", "image", "focal_length", "text", "resize", "side_view",
                                    "baseColorFactor", "rot_angle", "trans", "do_flip", "inv_trans"]
    d = {k: p.default for k, p in sig.parameters.items()}
    assert d["focal_length"] == 5000 and d["text"] is None and d["resize"] is None and d["side_view"] is False
    assert d["baseColorFactor"] == (1.0, 1.0, 0.9, 1.0) and d["rot_angle"] == 90
    assert d["trans"] is None and d["do_flip"] is None and d["inv_trans"] is None
    assert list(inspect.signature(MR.MeshRenderer.__init__).parameters)[:3] == ["self", "cfg", "faces"]
    R = MR.side_view_matrix(90)
    assert np.allclose(R @ np.array([1.0, 2.0, 0.0]), [0.0, 2.0, -1.0]) and np.allclose(R @ np.array([0.0, 0.0, 1.0]), [1.0, 0.0, 0.0])
    R30 = MR.side_view_matrix(30)
    assert np.allclose(R30 @ R30.T, np.eye(3)) and np.isclose(np.linalg.det(R30), 1.0) and np.allclose(R30[1], [0, 1, 0])
    assert np.isclose(R30[0, 0], np.cos(np.pi / 6)) and np.isclose(R30[0, 2], np.sin(np.pi / 6))
    import torch
    v = torch.tensor([[[1.0, 2.0, 0.0], [0.0, 0.0, 1.0]]])
    t = torch.tensor([[0.5, 0.25, 2.0]])
    got = MR.placed_vertices(v, t, side_view=True, rot_angle=90).numpy()
    assert got.dtype == np.float64 and np.allclose(got[0], [[0.5, 2.25, 1.0], [1.5, 0.25, 2.0]])
    assert np.array_equal(MR.placed_vertices(v, t).numpy()[0], v[0].double().numpy() + t[0].double().numpy())


def test_image_fusion_on_arrays():
    from hamer_yolo_amd import d_infer, infer
    assert d_infer.image_fusion is infer.image_fusion
    rng = np.random.default_rng(1)
    ori = rng.integers(1, 255, (6, 8, 4), dtype=np.uint8)
    a = np.zeros((6, 8, 4), np.uint8); a[1:3, 1:4] = (10, 0, 0, 255)
    b = np.zeros((6, 8, 4), np.uint8); b[2:5, 3:6] = (0, 0, 7, 255); b[0, 0, 3] = 255        # alpha alone does not count
    keep = ori.copy()
    got = infer.image_fusion(ori, [a, b])
    want = ori.copy()
    for im in (a, b):
        mask = np.any(im[:, :, :3] > 0, axis=-1)
        want = np.where(mask[:, :, None], im, want)
    assert np.array_equal(got, want) and np.array_equal(ori, keep)                            # a new array
    assert (got[2, 3] == (0, 0, 7, 255)).all() and (got[1, 1] == (10, 0, 0, 255)).all() and (got[0, 0] == ori[0, 0]).all()
    got3 = infer.image_fusion(ori[:, :, :3], [a, b])                                          # a 3-channel original
    assert got3.shape == (6, 8, 3) and np.array_equal(got3, want[:, :, :3])
    assert np.array_equal(infer.image_fusion(ori, []), ori)


def test_get_mesh_renderer_does_no_device_work():
    import torch
    from hamer_yolo_amd import synth
    from hamer_yolo_amd.hamer.utils.mesh_renderer import MeshRenderer
    from hamer_yolo_amd.infer import hamer_inference

    class _Mano:
        faces = synth.mano_params(seed=0)["faces"].numpy()

    class _Model:
        mano = _Mano()

    class _Cfg:
        class EXTRA:
            FOCAL_LENGTH = 5000
        class MODEL:
            IMAGE_SIZE = 256

    hi = hamer_inference.__new__(hamer_inference)                # the constructor loads a model onto the GPU
    hi.model, hi.cfg = _Model(), _Cfg
    before = torch.cuda.is_initialized()
    r = hi.get_mesh_renderer()
    assert isinstance(r, MeshRenderer) and hi.mano is _Model.mano
    assert r.faces.dtype == np.int32 and np.array_equal(r.faces, _Mano.faces) and r.focal_length == 5000
    assert r._faces_dev == {} and torch.cuda.is_initialized() == before
    assert callable(r.render_hands) and callable(hi.get_image)
