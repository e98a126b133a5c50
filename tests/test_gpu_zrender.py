"""GPU: the z-buffered renderer (hm_mesh_render) against the numpy statement of its rule (tests/zrender_rule.py), its
determinism properties, and the interface built on it (render.render_views, MeshRenderer, hamer_inference.get_image,
image_fusion, render.hand_maps_folder, render_folder(style="smooth")) end to end with synthetic weights."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import zrender_rule as ZR
from hamer_yolo_amd import lib as L
from hamer_yolo_amd import render, synth

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _surface(nu=26, nv=30, size=0.16):
    """A closed ellipsoid of MANO's size (780 vertices, 1500 faces) whose triangles join neighbouring vertices, as a real
    hand mesh's do (the surface topology of tools/bench_render.py)."""
    u = np.linspace(0.05, np.pi - 0.05, nu)[:, None]
    w = np.linspace(0, 2 * np.pi, nv, endpoint=False)[None, :]
    v = np.stack([0.5 * size * np.sin(u) * np.cos(w), 0.5 * size * np.cos(u) + 0 * w, 0.2 * size * np.sin(u) * np.sin(w)], -1)
    idx = np.arange(nu * nv).reshape(nu, nv)
    a, b, c, d = idx[:-1], np.roll(idx, -1, 1)[:-1], idx[1:], np.roll(idx, -1, 1)[1:]
    f = np.concatenate([np.stack([a, b, c], -1).reshape(-1, 3), np.stack([b, d, c], -1).reshape(-1, 3)])
    return v.reshape(-1, 3), f.astype(np.int32)


def _hand(seed, frame, H, W, z, right=True, off_screen=False, topology="surface", scale=1.0):
    """A hand-sized mesh placed in view `frame`: the surface topology, tilted so that its depth varies, or the synthetic
    MANO topology (778 vertices, random vertex triples: every face as large as the hand, full of interpenetrations)."""
    rng = np.random.default_rng(seed)
    if topology == "surface":
        v, f = _surface()
        a, b = rng.uniform(-0.6, 0.6, 2)
        Rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
        Ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
        v = v @ (Ry @ Rx).T * scale
    else:
        mp = synth.mano_params(seed=0)
        v, f = mp["v_template"].double().numpy() * scale, mp["faces"].numpy().astype(np.int32)
    if not right:
        v = v * np.array([-1.0, 1.0, 1.0])                                # mirrored, faces NOT flipped: shading is two-sided
    foc = 1000.0
    cx, cy = (rng.uniform(-0.1, 0.1) * W, rng.uniform(-0.1, 0.1) * H) if off_screen else \
        (rng.uniform(0.25, 0.75) * W, rng.uniform(0.25, 0.75) * H)
    t = np.array([(cx - W / 2) * z / foc, (cy - H / 2) * z / foc, z])
    return {"frame": frame, "vertices": v + t, "faces": f, "is_right": right}


def _K(H, W):
    return np.array([[1000.0, 0, W / 2], [0, 1000.0, H / 2], [0, 0, 1]])


def _scene(N, H, W, per_frame, seed, topology="surface", scale=1.0, z0=0.5):
    meshes = []
    for n in range(N):
        for k in range(per_frame):
            meshes.append(_hand(seed * 1000 + n * 10 + k, n, H, W, z=z0 + 0.03 * k, right=(k % 2 == 0), off_screen=(k == 2),
                                topology=topology, scale=scale))
    if per_frame >= 2:                                                     # two hands through each other
        c0, c1 = meshes[0]["vertices"].mean(0), meshes[1]["vertices"].mean(0)
        meshes[1]["vertices"] = meshes[1]["vertices"] - c1 + c0 + np.array([0.02, 0.01, 0.004])
    return meshes


def _oracle_meshes(meshes):
    out, f0 = [], 0
    for m in meshes:
        out.append(dict(m, face_id0=f0))
        f0 += len(m["faces"])
    return out


def _gpu(N, H, W, K, meshes, frames=None, **kw):
    fd = torch.from_numpy(frames).to(DEV) if frames is not None else None
    r = render.render_views(H, W, K, meshes, frames=fd, views=N, **kw)
    return {k: v.cpu().numpy() for k, v in r.items()}


def _compare(got, want, frames=None):
    """mesh label, coverage (alpha) and depth bits equal; colour within one per channel (fp64 sqrt)."""
    cov = want["face"] >= 0
    assert cov.any()
    assert np.array_equal(got["mesh_id"], want["mesh_id"]), f"{int((got['mesh_id'] != want['mesh_id']).sum())} labels differ"
    assert np.array_equal(got["rgba"][..., 3], want["rgba"][..., 3])
    gd, wd = got["depth"].view(np.uint32), want["depth"].view(np.uint32)
    assert np.array_equal(gd, wd), f"{int((gd != wd).sum())} depth values differ, largest step {int(np.abs(gd.astype(np.int64) - wd.astype(np.int64)).max())} ulp"
    assert int(np.abs(got["rgba"].astype(int) - want["rgba"].astype(int)).max()) <= 1
    assert np.array_equal(got["rgba"][~cov], want["rgba"][~cov])
    if frames is not None:
        assert np.array_equal(got["out"][~cov], frames[~cov])
        assert np.array_equal(got["out"][cov], got["rgba"][..., 2::-1][cov])
        assert int(np.abs(got["out"].astype(int) - want["out"].astype(int)).max()) <= 1


@pytest.mark.parametrize("N,H,W,per_frame", [(1, 1080, 1920, 1), (1, 1080, 1920, 4), (2, 479, 641, 3)])
def test_parity_with_the_rule_surface_topology(N, H, W, per_frame):
    meshes = _scene(N, H, W, per_frame, seed=N + H + per_frame)
    frames = np.stack([synth.frame_u8(H, W, seed=n).numpy() for n in range(N)])
    got = _gpu(N, H, W, _K(H, W), meshes, frames=frames)
    want = ZR.render(N, H, W, _K(H, W), _oracle_meshes(meshes), frames=frames)
    _compare(got, want, frames)
    for n in range(N):                                                     # every on-screen hand is seen
        assert len(np.unique(want["mesh_id"][n])) >= min(per_frame, 2) + 1


def test_parity_synthetic_mano_topology_and_a_hand_behind_znear():
    """The synthetic MANO topology (every face as large as the hand: interpenetrations everywhere) on a small frame, two
    hands on top of each other; and in view 1 a surface hand so close that part of it lies nearer than znear: its faces with
    a corner there are dropped whole (no clipping), the others stay."""
    N, H, W = 2, 200, 300
    meshes = _scene(1, H, W, 2, seed=7, topology="synthetic", scale=0.35)
    near = _hand(5, 1, H, W, z=0.055, scale=0.15)
    assert (near["vertices"][:, 2] < 0.05).sum() > 50 and (near["vertices"][:, 2] > 0.055).sum() > 50
    meshes.append(near)
    K = np.stack([_K(H, W), np.array([[300.0, 0, W / 2], [0, 300.0, H / 2], [0, 0, 1]])])       # a camera per view
    bg, base = (9, 8, 7, 0), (0.25, 1.0, 0.5)
    got = _gpu(N, H, W, K, meshes, bg=bg, base_color=base)
    want = ZR.render(N, H, W, K, _oracle_meshes(meshes), bg_rgba=bg, base_rgb=base)
    _compare(got, want)
    assert set(np.unique(want["mesh_id"][0])) == {-1, 0, 1} and set(np.unique(want["mesh_id"][1])) == {-1, 2}
    one = _gpu(N, H, W, K, meshes, znear=0.01)                       # with a nearer plane more of it is drawn
    assert (one["mesh_id"][1] == 2).sum() > (got["mesh_id"][1] == 2).sum()
    _compare(one, ZR.render(N, H, W, K, _oracle_meshes(meshes), znear=0.01))


def test_winning_face_one_mesh_per_face():
    """Every face a mesh of its own (its three vertices copied), so that the label map names the winning FACE; also more
    meshes than one launch's argument block holds."""
    H, W = 240, 320
    a = _hand(1, 0, H, W, z=0.5)
    b = _hand(2, 0, H, W, z=0.5)
    b["vertices"] = b["vertices"] - b["vertices"].mean(0) + a["vertices"].mean(0) + np.array([0.01, 0.0, 0.0])
    meshes = []
    for h in (a, b):
        for row in h["faces"][::3]:
            meshes.append({"frame": 0, "vertices": h["vertices"][row], "faces": np.array([[0, 1, 2]], np.int32)})
    assert len(meshes) == 1000
    got = _gpu(1, H, W, _K(H, W), meshes)
    want = ZR.render(1, H, W, _K(H, W), _oracle_meshes(meshes))
    assert np.array_equal(want["mesh_id"], want["face"].astype(np.int32))
    _compare(got, want)
    assert len(np.unique(got["mesh_id"])) > 200


# ------------------------------------------------------------------ determinism, at the C ABI
def _tables(meshes):
    verts = torch.from_numpy(np.concatenate([m["vertices"] for m in meshes])).to(DEV)
    faces = torch.from_numpy(np.concatenate([m["faces"] for m in meshes])).to(DEV)
    rows, v0, f0 = [], 0, 0
    for m in meshes:
        r = L.Mesh()
        r.frame, r.v0, r.nv, r.f0, r.nf = m["frame"], v0, len(m["vertices"]), f0, len(m["faces"])
        rows.append(r); v0 += r.nv; f0 += r.nf
    return verts, faces, rows


def _abi(N, H, W, K, verts, faces, table, ws, want=("rgba", "depth", "mesh_id"), frames=None):
    o = {"rgba": torch.empty(N, H, W, 4, dtype=torch.uint8, device=DEV) if "rgba" in want else None,
         "depth": torch.empty(N, H, W, dtype=torch.float32, device=DEV) if "depth" in want else None,
         "mesh_id": torch.empty(N, H, W, dtype=torch.int32, device=DEV) if "mesh_id" in want else None,
         "out": torch.empty_like(frames) if frames is not None else None}
    Kh = np.ascontiguousarray(np.broadcast_to(np.asarray(K, np.float64), (N, 3, 3)))
    L.check(L.load().hm_mesh_render(N, H, W, Kh.ctypes.data_as(C.POINTER(C.c_double)), verts.data_ptr(), verts.shape[0],
                                    faces.data_ptr(), faces.shape[0], table, len(table), None, None, 0.05, L.ptr(frames),
                                    L.ptr(o["out"]), L.ptr(o["rgba"]), L.ptr(o["depth"]), L.ptr(o["mesh_id"]), ws.data_ptr(),
                                    ws.numel(), L.current_stream()), "hm_mesh_render")
    return {k: v.cpu().numpy() for k, v in o.items() if v is not None}


@pytest.mark.parametrize("H,W", [(200, 300), (120, 161)])               # 16-byte rows and rows that are not
def test_deterministic_order_independent_and_workspace_reuse(H, W):
    N = 3
    meshes = _scene(N, H, W, 4, seed=5, scale=0.5)
    meshes[3]["vertices"] = meshes[0]["vertices"].copy()                   # exact depth ties across meshes of view 0
    verts, faces, rows = _tables(meshes)
    need = L.load().hm_mesh_render_workspace_bytes(N, H, W, verts.shape[0], len(rows), faces.shape[0])
    ws = torch.full((need,), 255, dtype=torch.uint8, device=DEV)
    ident = list(range(len(rows)))
    perm = [int(i) for i in np.random.default_rng(0).permutation(len(rows))]
    frames = torch.from_numpy(np.stack([synth.frame_u8(H, W, seed=n).numpy() for n in range(N)])).to(DEV)
    outs = []
    for p in (ident, ident, perm):
        table = (L.Mesh * len(rows))(*[rows[i] for i in p])
        outs.append(_abi(N, H, W, _K(H, W), verts, faces, table, ws, frames=frames))     # the same workspace every time
        assert bool((ws[:N * H * W * 8] == 255).all())                    # every key written was reset
    a, b, c = outs
    for k in a:
        assert np.array_equal(a[k], b[k])                                  # two calls, the same bytes
    assert np.array_equal(a["rgba"], c["rgba"]) and np.array_equal(a["depth"].view(np.uint32), c["depth"].view(np.uint32))
    assert np.array_equal(a["out"], c["out"])
    inv = np.empty(len(perm), np.int32)
    inv[perm] = np.arange(len(perm), dtype=np.int32)                       # table row k holds mesh perm[k]
    cov = a["mesh_id"] >= 0
    assert cov.any() and np.array_equal(c["mesh_id"][cov], inv[a["mesh_id"][cov]]) and (c["mesh_id"][~cov] == -1).all()
    assert (a["mesh_id"][0] == 0).any() and not (a["mesh_id"][0] == 3).any()          # the tie went to the lower face row
    # one output alone has the bytes it has among all
    table = (L.Mesh * len(rows))(*rows)
    for name in ("rgba", "depth", "mesh_id"):
        alone = _abi(N, H, W, _K(H, W), verts, faces, table, ws, want=(name,))
        assert list(alone) == [name] and np.array_equal(alone[name].view(np.uint8), a[name].view(np.uint8))
    only_out = _abi(N, H, W, _K(H, W), verts, faces, table, ws, want=(), frames=frames)
    assert list(only_out) == ["out"] and np.array_equal(only_out["out"], a["out"])
    # frames + out against rgba
    fr = frames.cpu().numpy()
    assert np.array_equal(a["out"][cov], a["rgba"][..., 2::-1][cov]) and np.array_equal(a["out"][~cov], fr[~cov])
    # a view alone has the bytes it has inside the batch
    for n in range(N):
        mine = [dict(m, frame=0) for m in meshes if m["frame"] == n]
        v1, f1, r1 = _tables(mine)
        ws1 = torch.full((L.load().hm_mesh_render_workspace_bytes(1, H, W, v1.shape[0], len(r1), f1.shape[0]),), 255,
                         dtype=torch.uint8, device=DEV)
        solo = _abi(1, H, W, _K(H, W), v1, f1, (L.Mesh * len(r1))(*r1), ws1)
        assert np.array_equal(solo["rgba"][0], a["rgba"][n]) and np.array_equal(solo["depth"][0].view(np.uint32), a["depth"][n].view(np.uint32))
        first = min(i for i, m in enumerate(meshes) if m["frame"] == n)
        assert np.array_equal(np.where(solo["mesh_id"][0] >= 0, solo["mesh_id"][0] + first, -1), a["mesh_id"][n])


def _exact(got, want):
    """Every output byte equal to the rule's: labels, depth bits and colour."""
    assert np.array_equal(got["mesh_id"], want["mesh_id"]), f"{int((got['mesh_id'] != want['mesh_id']).sum())} labels differ"
    assert np.array_equal(got["depth"].view(np.uint32), want["depth"].view(np.uint32))
    step = int(np.abs(got["rgba"].astype(int) - want["rgba"].astype(int)).max())
    print("largest colour step", step)
    assert np.array_equal(got["rgba"], want["rgba"]), f"colour differs by up to {step}"


def test_more_meshes_than_one_setup_launch():
    """50 small closed meshes in 2 views: the mesh table is walked in two argument blocks (48 + 2), so meshes 48 and 49 get
    their rows from the second block's `first`.  Mesh 49 stands in front of mesh 0, and mesh 25 has 308 faces, so the raster
    culls it in two chunks of 256."""
    N, H, W, foc = 2, 48, 80, 100.0
    K = np.array([[foc, 0, W / 2], [0, foc, H / 2], [0, 0, 1]])
    meshes = []
    for i in range(50):
        v, f = _surface(nu=12, nv=14, size=0.09) if i == 25 else _surface(nu=4, nv=6, size=0.03 if i == 49 else 0.06)
        a = 0.1 * i
        Rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
        slot = 0 if i == 49 else i // 2                                     # 7 x 4 places per view; mesh 49 on mesh 0's
        z = 0.42 if i == 49 else 0.5 + 0.002 * i
        cx, cy = 7 + 11 * (slot % 7), 7 + 11 * (slot // 7)
        t = np.array([(cx - W / 2) * z / foc, (cy - H / 2) * z / foc, z])
        meshes.append({"frame": 0 if i == 49 else i % 2, "vertices": v @ Rx.T + t, "faces": f})
    assert len(meshes[25]["faces"]) > 256
    got = _gpu(N, H, W, K, meshes)
    want = ZR.render(N, H, W, K, _oracle_meshes(meshes))
    seen = set(np.unique(want["mesh_id"]))
    assert {0, 25, 47, 48, 49} <= seen and len(seen) >= 45
    _exact(got, want)


def test_both_renderers_share_one_key_buffer():
    """overlay, z-buffer, overlay, z-buffer on one stream and one (N, H, W): the calls share the workspace's key buffer (the
    second call allocates the larger workspace; the third and fourth find the keys the call before them left), each result
    equals its own rule and the same call on a fresh workspace.  W % 4 != 0: the one-pixel resolve."""
    import render_rule as RR
    N, H, W = 3, 120, 161
    meshes = _scene(N, H, W, 2, seed=11, scale=0.5)
    frames = np.stack([synth.frame_u8(H, W, seed=20 + n).numpy() for n in range(N)])
    fd = torch.from_numpy(frames).to(DEV)
    render.release_workspaces()

    def overlay():
        return render.overlay_frames(fd, _K(H, W), meshes).cpu().numpy()

    def zbuffer():
        return _gpu(N, H, W, _K(H, W), meshes)
    a1, z1, a2, z2 = overlay(), zbuffer(), overlay(), zbuffer()
    assert len(render._ws) == 1
    ws = next(iter(render._ws.values()))[0]
    assert bool((ws[:N * H * W * 8] == 255).all())                        # every key written was reset
    want_a = RR.overlay(frames, _K(H, W), [dict(m, color=(0, 255, 0)) for m in _oracle_meshes(meshes)])
    want_z = ZR.render(N, H, W, _K(H, W), _oracle_meshes(meshes))
    assert (want_a != frames).any() and (want_z["face"] >= 0).any()
    render.release_workspaces()
    fresh_a = overlay()
    render.release_workspaces()
    fresh_z = zbuffer()
    render.release_workspaces()
    for a in (a1, a2, fresh_a):
        assert np.array_equal(a, want_a), f"{int((a != want_a).any(-1).sum())} pixels differ"
    for z in (z1, z2):
        for k in fresh_z:
            assert np.array_equal(z[k].view(np.uint8), fresh_z[k].view(np.uint8))
    _exact(fresh_z, want_z)


def test_render_views_arguments():
    m = _hand(0, 0, 64, 96, 0.5, scale=0.2)
    with pytest.raises(ValueError):
        render.render_views(64, 96, _K(64, 96), [m], outputs=("rgba", "normals"))
    with pytest.raises(ValueError):
        render.render_views(64, 96, _K(64, 96), [m], outputs=())
    with pytest.raises(ValueError):
        render.render_views(64, 96, np.stack([_K(64, 96)] * 2), [m], views=3)
    with pytest.raises(L.HipLibraryError):
        render.render_views(64, 96, _K(64, 96), [m], znear=0.0)
    Kbad = _K(64, 96); Kbad[2, 2] = 2.0
    with pytest.raises(L.HipLibraryError):
        render.render_views(64, 96, Kbad, [m])
    r = render.render_views(64, 96, _K(64, 96), [m], outputs=("depth",))
    assert list(r) == ["depth"] and tuple(r["depth"].shape) == (1, 64, 96) and bool((r["depth"] > 0).any())
    empty = render.render_views(64, 96, _K(64, 96), [], bg=(1, 2, 3, 4))
    assert bool((empty["mesh_id"] == -1).all()) and bool((empty["depth"] == 0).all())
    assert bool((empty["rgba"] == torch.tensor([1, 2, 3, 4], dtype=torch.uint8, device=DEV)).all())
    render.release_workspaces()


# ------------------------------------------------------------------ end to end, synthetic weights
class _Cfg:
    ckpt_path = "synthetic:0"
    model_cfg = None
    use_onnx = False
    onnx_path = None


class _FixedDetector:
    def __init__(self, dets):
        self.dets = dets

    def detect(self, image):
        return [None], [self.dets]


@pytest.fixture(scope="module")
def hi():
    from hamer_yolo_amd.infer import hamer_inference
    return hamer_inference(_Cfg)


H2, W2 = 360, 640
DETS = [["right", [150.0, 100.0, 230.0, 190.0]], ["left", [400.0, 160.0, 470.0, 250.0]]]


def test_get_image_and_image_fusion(hi):
    from hamer_yolo_amd.hamer.utils.mesh_renderer import MeshRenderer, placed_vertices
    from hamer_yolo_amd.infer import image_fusion
    renderer = hi.get_mesh_renderer()
    assert isinstance(renderer, MeshRenderer)
    frame = synth.frame_u8(H2, W2, seed=3).numpy()
    images = hi.get_image(DETS, frame, renderer)
    assert len(images) == 2 and all(im.shape == (H2, W2, 4) and im.dtype == np.uint8 for im in images)
    assert len(hi.get_image([DETS], frame, renderer)) == 2                  # nested once, as the detector returns them
    assert hi.get_image([], frame, renderer) == []
    out, _ = hi.estimate_from_rgb(frame, DETS)
    verts = out["pred_vertices"].float().clone()
    verts[:, :, 0] *= (1.0 - 2.0 * out["do_flip"].view(-1, 1))
    assert out["do_flip"].cpu().tolist() == [0.0, 1.0]
    placed = placed_vertices(verts, out["pred_cam_t_full"])
    foc = float(out["focal_length"].flatten()[0])
    K = np.array([[foc, 0, W2 / 2], [0, foc, H2 / 2], [0, 0, 1]])
    faces = torch.as_tensor(np.asarray(hi.mano.faces, np.int32), device=placed.device)
    for i, im in enumerate(images):
        one = render.render_views(H2, W2, K, [{"frame": 0, "vertices": placed[i], "faces": faces}], outputs=("rgba",))
        assert np.array_equal(im, one["rgba"][0].cpu().numpy()) and (im[..., 3] == 255).any()
        call = renderer(verts[i], out["pred_cam_t_full"][i], frame, focal_length=out["focal_length"])   # the reference's call
        assert call.dtype == np.float32 and call.shape == (H2, W2, 4) and np.array_equal(call, im.astype(np.float32) / 255.0)
    side = renderer(verts[0], out["pred_cam_t_full"][0], frame, focal_length=foc, side_view=True)
    want = render.render_views(H2, W2, K, [{"frame": 0, "vertices": placed_vertices(verts[:1], out["pred_cam_t_full"][:1], True, 90)[0],
                                            "faces": faces}], outputs=("rgba",))["rgba"][0].cpu().numpy()
    assert np.array_equal(side, want.astype(np.float32) / 255.0) and not np.array_equal(want, images[0])
    # fusion against the composite of both hands in one view.  Fusion lets the later image win and the z-buffer the nearer
    # face, so the two may differ where both hands have colour, and only there
    both = render.render_views(H2, W2, K, [{"frame": 0, "vertices": placed[i], "faces": faces} for i in range(2)],
                               outputs=("rgba",))["rgba"][0].cpu().numpy()
    ori = np.concatenate([frame, np.full((H2, W2, 1), 255, np.uint8)], -1)
    fused = image_fusion(ori, images)
    colour = [np.any(im[:, :, :3] > 0, -1) for im in images]
    single, overlap = colour[0] ^ colour[1], colour[0] & colour[1]
    assert colour[0].any() and colour[1].any() and np.array_equal(fused[single], both[single])
    assert np.array_equal(fused[overlap], images[1][overlap])              # where both have colour the later image wins
    none = ~(colour[0] | colour[1])
    assert np.array_equal(fused[none], ori[none])
    render.release_workspaces()


def _decode(path):
    from PIL import Image
    with Image.open(path) as im:
        return np.asarray(im.convert("RGB"))[:, :, ::-1]


def test_hand_maps_and_smooth_folder(hi, tmp_path):
    from PIL import Image
    from hamer_yolo_amd.infer import get_bbox_from_npy, process_batch_manopara, process_batch_manopara_with_mask
    img_dir, npy_dir, map_dir, out_dir, rec_dir = (tmp_path / d for d in ("rgb", "npy", "maps", "smooth", "masked"))
    img_dir.mkdir()
    H, W = 240, 320
    frames = {}
    for i in range(3):
        fr = synth.frame_u8(H, W, seed=60 + i).numpy()
        frames[f"f{i}"] = fr
        Image.fromarray(fr[:, :, ::-1]).save(img_dir / f"f{i}.png")
    dets = [["right", [60.0, 50.0, 120.0, 120.0]], ["left", [190.0, 90.0, 250.0, 160.0]]]
    process_batch_manopara(str(img_dir), str(npy_dir), None, hamer=hi, detector=_FixedDetector(dets))
    n = render.hand_maps_folder(str(img_dir), str(npy_dir), str(map_dir), hi, label=3, frames_per_pass=2)       # passes 2 + 1
    assert n == 3 and render._ws == {}
    assert sorted(os.listdir(map_dir)) == sorted([f"f{i}.npy" for i in range(3)] + [f"f{i}_maps.npz" for i in range(3)])
    assert render.render_folder(str(img_dir), str(npy_dir), str(out_dir), hi, style="smooth", ext=".png", frames_per_pass=2) == 3
    assert sorted(os.listdir(out_dir)) == ["f0.png", "f1.png", "f2.png"]
    K = render.default_camera(H, W, hi.cfg)
    faces = np.asarray(hi.mano.faces, np.int32)
    for name, fr in frames.items():
        data = np.load(npy_dir / f"{name}.npy", allow_pickle=True).item()
        hands = [data[t] for t in ("right", "left") if data[t] is not None]
        assert len(hands) == 2
        cam = render.camera_vertices(hi, hands).cpu().numpy().astype(np.float64)
        meshes = [{"frame": 0, "vertices": cam[j], "faces": faces, "face_id0": j * len(faces)} for j in range(len(hands))]
        want = ZR.render(1, H, W, K, meshes, frames=fr[None])
        sil = want["face"][0] >= 0
        assert sil.any()
        mask = np.load(map_dir / f"{name}.npy")
        assert mask.dtype == np.uint8 and mask.shape == (H, W) and np.array_equal(mask, np.where(sil, 3, 0).astype(np.uint8))
        rows, cols = np.nonzero(sil)
        assert get_bbox_from_npy(str(map_dir / f"{name}.npy")) == [float(cols.min()), float(rows.min()), float(cols.max()), float(rows.max())]
        maps = np.load(map_dir / f"{name}_maps.npz")
        assert maps["depth"].dtype == np.float32 and maps["hand"].dtype == np.int8
        assert np.array_equal(maps["hand"], want["mesh_id"][0].astype(np.int8))
        assert np.array_equal(maps["depth"].view(np.uint32), want["depth"][0].view(np.uint32))
        for j in range(len(hands)):
            d = maps["depth"][maps["hand"] == j]
            assert len(d) == 0 or (d.min() >= np.float32(cam[j][:, 2].min()) and d.max() <= np.float32(cam[j][:, 2].max()))
        assert (maps["depth"][maps["hand"] == -1] == 0).all()
        got = _decode(out_dir / f"{name}.png")
        assert np.array_equal(got[~sil], fr[~sil]) and int(np.abs(got.astype(int) - want["out"][0].astype(int)).max()) <= 1
    process_batch_manopara_with_mask(str(img_dir), str(map_dir), str(rec_dir), hamer=hi)
    assert sorted(os.listdir(rec_dir)) == ["f0.npy", "f1.npy", "f2.npy"]
    rec = np.load(rec_dir / "f0.npy", allow_pickle=True).item()
    assert rec["right"] is not None and rec["left"] is None


def test_driver_options_reach_the_folder_paths(hi, tmp_path, monkeypatch):
    """``--hand-maps`` / ``--hand-label`` / ``--render-style smooth`` through infer.main, on the module's model and a fixed
    detector."""
    from PIL import Image
    from hamer_yolo_amd import infer
    img_dir, npy_dir, map_dir, out_dir = (tmp_path / d for d in ("rgb", "npy", "maps", "smooth"))
    img_dir.mkdir()
    for i in range(2):
        Image.fromarray(synth.frame_u8(240, 320, seed=80 + i).numpy()[:, :, ::-1]).save(img_dir / f"g{i}.png")
    dets = [["right", [60.0, 50.0, 120.0, 120.0]]]
    real = infer.process_batch_manopara
    monkeypatch.setattr(infer, "hamer_inference", lambda cfg: hi)
    monkeypatch.setattr(infer, "process_batch_manopara", lambda i, o, k, hamer=None, rank=0, world=1:
                        real(i, o, k, hamer=hamer, detector=_FixedDetector(dets), rank=rank, world=world))
    infer.main(["--input", str(img_dir), "--output", str(npy_dir), "--hand-maps", str(map_dir), "--hand-label", "5",
                "--render", str(out_dir), "--render-style", "smooth"])
    assert sorted(os.listdir(map_dir)) == ["g0.npy", "g0_maps.npz", "g1.npy", "g1_maps.npz"]
    assert sorted(os.listdir(out_dir)) == ["g0.jpg", "g1.jpg"]
    for stem in ("g0", "g1"):
        mask, maps = np.load(map_dir / f"{stem}.npy"), np.load(map_dir / f"{stem}_maps.npz")
        assert mask.shape == (240, 320) and set(np.unique(mask)) == {0, 5}
        assert np.array_equal(mask == 5, maps["hand"] == 0) and np.array_equal(mask == 5, maps["depth"] > 0)
