"""GPU: the mesh overlay kernels (hm_mesh_overlay) against the numpy statement of the drawing rule (tests/render_rule.py), and
the folder paths built on them (render.render_folder, hamer.reconstruct.main) end to end with synthetic weights."""
import os

import numpy as np
import pytest
import torch

import render_rule as RR
from hamer_yolo_amd import lib as L
from hamer_yolo_amd import render, synth

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LEFT_COLOR = (255, 0, 0)


def _hand(seed, frame, H, W, scale, z, right=True, off_screen=False):
    """A MANO-shaped mesh (778 vertices, the synthetic topology: long random triangles) placed in frame `frame`."""
    mp = synth.mano_params(seed=0)
    rng = np.random.default_rng(seed)
    v = mp["v_template"].double().numpy() * scale
    if not right:
        v[:, 0] = -v[:, 0]
    f = 1000.0
    cx, cy = (rng.uniform(-0.1, 0.1) * W, rng.uniform(-0.1, 0.1) * H) if off_screen else \
        (rng.uniform(0.2, 0.8) * W, rng.uniform(0.2, 0.8) * H)
    t = np.array([(cx - W / 2) * z / f, (cy - H / 2) * z / f, z])
    return {"frame": frame, "vertices": v + t, "faces": mp["faces"].numpy().astype(np.int32), "is_right": right}


def _K(H, W):
    return np.array([[1000.0, 0, W / 2], [0, 1000.0, H / 2], [0, 0, 1]])


def _oracle_meshes(meshes):
    out, f0 = [], 0
    for m in meshes:
        out.append(dict(m, face_id0=f0, color=m.get("color") or ((0, 255, 0) if m.get("is_right", True) else LEFT_COLOR)))
        f0 += len(m["faces"])
    return out


def _gpu(frames, K, meshes, style="flat"):
    out = render.overlay_frames(torch.from_numpy(frames).to(DEV), K, meshes, style=style, color_left=LEFT_COLOR)
    return out.cpu().numpy()


def _scene(N, H, W, per_frame, seed, scale=0.6):
    frames = np.stack([synth.frame_u8(H, W, seed=seed + n).numpy() for n in range(N)])
    meshes = []
    for n in range(N):
        for k in range(per_frame):
            meshes.append(_hand(seed * 1000 + n * 10 + k, n, H, W, scale, z=0.5 + 0.05 * k, right=(k % 2 == 0),
                                off_screen=(k == 2)))
    return frames, meshes


@pytest.mark.parametrize("N,H,W,per_frame,scale", [(1, 1080, 1920, 1, 1.0), (1, 1080, 1920, 4, 0.8), (2, 479, 641, 3, 0.5),
                                                   (64, 64, 64, 2, 0.08), (64, 120, 160, 4, 0.15)])
def test_flat_bit_exact(N, H, W, per_frame, scale):
    frames, meshes = _scene(N, H, W, per_frame, seed=N + H, scale=scale)
    got = _gpu(frames, _K(H, W), meshes)
    want = RR.overlay(frames, _K(H, W), _oracle_meshes(meshes))
    assert (got != frames).any()
    assert np.array_equal(got, want), f"{int((got != want).any(-1).sum())} pixels differ"


def test_faces_behind_camera_and_overlapping_hands():
    H, W = 240, 320
    frames = np.stack([synth.frame_u8(H, W, seed=9).numpy()] * 2)
    right = _hand(1, 0, H, W, 1.5, 0.6, right=True)
    left = _hand(1, 0, H, W, 1.5, 0.62, right=False)                         # on top of each other, different colours
    behind = _hand(2, 1, H, W, 1.5, 0.6)
    behind["vertices"] = behind["vertices"] - np.array([0, 0, 0.6 + behind["vertices"][:, 2].min() - 0.01]) * 1.0
    behind["vertices"][::2, 2] -= 0.05                                        # some corners behind the camera, some not
    meshes = [right, left, behind]
    got = _gpu(frames, _K(H, W), meshes)
    want = RR.overlay(frames, _K(H, W), _oracle_meshes(meshes))
    assert np.array_equal(got, want)
    colours = {tuple(c) for c in got[0][(got[0] != frames[0]).any(-1)].reshape(-1, 3)}
    assert len(colours) > 2


def _abi(frames_d, K, verts, faces, table, out, ws):
    N, H, W, _ = frames_d.shape
    L.check(L.load().hm_mesh_overlay(frames_d.data_ptr(), N, H, W, K.data_ptr(), verts.data_ptr(), verts.shape[0], faces.data_ptr(),
                                     faces.shape[0], table, len(table), L.HM_STYLE_FLAT, 0.6, out.data_ptr(), ws.data_ptr(),
                                     ws.numel(), L.current_stream()), "hm_mesh_overlay")


def test_deterministic_order_independent_and_workspace_reuse():
    N, H, W = 3, 200, 300
    frames, meshes = _scene(N, H, W, 4, seed=5, scale=0.4)
    for m in meshes[1:4]:                                                    # exact depth ties across meshes of frame 0
        m["vertices"] = meshes[0]["vertices"].copy()
    verts = torch.from_numpy(np.concatenate([m["vertices"] for m in meshes])).to(DEV)
    faces = torch.from_numpy(np.concatenate([m["faces"] for m in meshes])).to(DEV)
    rows, v0, f0 = [], 0, 0
    for i, m in enumerate(meshes):
        r = L.Mesh()
        r.frame, r.v0, r.nv, r.f0, r.nf = m["frame"], v0, len(m["vertices"]), f0, len(m["faces"])
        r.color_bgr[:] = (i * 20 % 256, 255 - i * 10, (i * 77) % 256)
        rows.append(r); v0 += r.nv; f0 += r.nf
    frames_d = torch.from_numpy(frames).to(DEV)
    K = torch.from_numpy(np.stack([_K(H, W)] * N)).to(DEV)
    need = L.load().hm_mesh_overlay_workspace_bytes(N, H, W, len(rows), f0)
    ws = torch.full((need,), 255, dtype=torch.uint8, device=DEV)
    outs = []
    for perm in (list(range(len(rows))), list(range(len(rows))), list(np.random.default_rng(0).permutation(len(rows)))):
        table = (L.Mesh * len(rows))(*[rows[i] for i in perm])
        out = torch.empty_like(frames_d)
        _abi(frames_d, K, verts, faces, table, out, ws)                      # the same workspace every time: keys reset
        outs.append(out.cpu().numpy())
    want = RR.overlay(frames, _K(H, W), [dict(m, face_id0=int(rows[i].f0), color=tuple(rows[i].color_bgr)) for i, m in enumerate(meshes)])
    for o in outs:
        assert np.array_equal(o, want)
    assert bool((ws[:N * H * W * 8] == 255).all())                         # every key written was reset


def test_shaded_within_one():
    H, W = 479, 641
    frames, meshes = _scene(2, H, W, 3, seed=3, scale=0.6)
    got = _gpu(frames, _K(H, W), meshes, style="shaded")
    want = RR.overlay(frames, _K(H, W), _oracle_meshes(meshes), style="shaded")
    ref_flat = RR.overlay(frames, _K(H, W), _oracle_meshes(meshes), alpha=1.0)
    covered = (ref_flat != frames).any(-1) | (want != frames).any(-1)
    assert covered.any()
    assert np.array_equal(got[~covered], frames[~covered])
    assert int(np.abs(got.astype(int) - want.astype(int)).max()) <= 1


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


def _decode(path):
    from PIL import Image
    with Image.open(path) as im:
        return np.asarray(im.convert("RGB"))[:, :, ::-1]


@pytest.mark.parametrize("with_k", [False, True])
def test_render_folder_and_reconstruct_main(hi, tmp_path, with_k):
    from PIL import Image
    from hamer_yolo_amd.hamer import reconstruct
    from hamer_yolo_amd.hamer.reconstruct import load_obj
    from hamer_yolo_amd.infer import process_batch_manopara, reconstruct_and_save_obj_with_wrapper
    img_dir, npy_dir, out_dir, obj_dir = (tmp_path / d for d in ("rgb", "npy", "render", "obj"))
    img_dir.mkdir()
    H, W = 1080, 1920
    frames = {}
    for i in range(3):
        fr = synth.frame_u8(H, W, seed=40 + i).numpy()
        frames[f"f{i}"] = fr
        Image.fromarray(fr[:, :, ::-1]).save(img_dir / f"f{i}.png")
    dets = [["right", [700.0, 400.0, 900.0, 640.0]], ["left", [1000.0, 450.0, 1180.0, 660.0]]]
    K = np.array([[1400.0, 0, 960], [0, 1400.0, 540], [0, 0, 1]], np.float32) if with_k else None
    process_batch_manopara(str(img_dir), str(npy_dir), K, hamer=hi, detector=_FixedDetector(dets))
    n = render.render_folder(str(img_dir), str(npy_dir), str(out_dir), hi, K, ext=".png", frames_per_pass=2)   # passes 2 + 1
    assert render._ws == {}                                                  # the workspaces are released after the folder
    assert n == 3 and sorted(os.listdir(out_dir)) == ["f0.png", "f1.png", "f2.png"]
    reconstruct_and_save_obj_with_wrapper(str(npy_dir), str(obj_dir), hi)
    Kd = np.asarray(K, np.float64) if with_k else render.default_camera(H, W, hi.cfg)
    faces = np.asarray(hi.mano.faces, np.int32)
    for name, fr in frames.items():
        data = np.load(npy_dir / f"{name}.npy", allow_pickle=True).item()
        hands = [data[t] for t in ("right", "left") if data[t] is not None]
        cam = render.camera_vertices(hi, hands).cpu().numpy().astype(np.float64)
        obj_v, obj_f = load_obj(str(obj_dir / f"{name}.obj"))
        assert np.abs(obj_v - cam.reshape(-1, 3)).max() <= 1e-6
        meshes = [{"frame": 0, "vertices": cam[j], "faces": faces, "face_id0": j * len(faces)} for j in range(len(hands))]
        want = RR.overlay(fr[None], Kd, meshes)[0]
        got = _decode(out_dir / f"{name}.png")
        assert (want != fr).any() and np.array_equal(got, want)
    if with_k:
        kfile = tmp_path / "K.txt"
        np.savetxt(kfile, K)
        rdir = tmp_path / "recon"
        assert reconstruct.main(["--img_dir", str(img_dir), "--obj_dir", str(obj_dir), "--intrinsics", str(kfile),
                                 "--out_dir", str(rdir), "--ext", ".png"], frames_per_pass=2) == 3
        for name, fr in frames.items():
            obj_v, obj_f = load_obj(str(obj_dir / f"{name}.obj"))
            want = RR.overlay(fr[None], np.loadtxt(kfile), [{"frame": 0, "vertices": obj_v, "faces": obj_f}])[0]
            assert np.array_equal(_decode(rdir / f"{name}.png"), want)


def test_project_and_draw_matches_rule():
    from hamer_yolo_amd.hamer.reconstruct import project_and_draw
    H, W = 479, 641
    frames, meshes = _scene(1, H, W, 1, seed=11, scale=0.7)
    m = meshes[0]
    got = project_and_draw(frames[0], m["vertices"], m["faces"], _K(H, W), alpha=0.6, color=(0, 0, 255))
    want = RR.overlay(frames, _K(H, W), [dict(m, color=(0, 0, 255))])[0]
    assert np.array_equal(got, want) and (got != frames[0]).any()


def test_default_camera_is_the_records_camera(hi):
    """Records made without intrinsics carry the camera translation of infer._estimate's no-intrinsics branch; the same
    hands estimated WITH render.default_camera as intrinsics must get the same translation (focal length and principal
    point both enter it), on a frame that is not square."""
    H, W = 1080, 1920
    frame = synth.frame_u8(H, W, seed=7).numpy()
    dets = [["right", [300.0, 200.0, 520.0, 430.0]], ["left", [1300.0, 600.0, 1500.0, 820.0]]]
    none, _ = hi.estimate_from_rgb(frame, dets, None)
    K = render.default_camera(H, W, hi.cfg)
    assert K[0, 2] == W / 2 and K[1, 2] == H / 2
    withk, _ = hi.estimate_from_rgb(frame, dets, K.astype(np.float32))
    a, b = none["pred_cam_t_full"].cpu().numpy(), withk["pred_cam_t_full"].cpu().numpy()
    np.testing.assert_allclose(a, b, rtol=1e-6, atol=1e-7)
    swapped = K.copy(); swapped[0, 2], swapped[1, 2] = H / 2, W / 2                   # a wrong principal point is caught
    wrong, _ = hi.estimate_from_rgb(frame, dets, swapped.astype(np.float32))
    assert np.abs(wrong["pred_cam_t_full"].cpu().numpy() - a).max() > 1e-3


def test_overlay_rejects_a_mismatched_out():
    frames = torch.zeros(2, 16, 24, 3, dtype=torch.uint8, device=DEV)
    m = _hand(0, 0, 16, 24, 0.05, 0.5)
    for bad in (torch.empty(1, 16, 24, 3, dtype=torch.uint8, device=DEV), torch.empty(2, 16, 24, 3, device=DEV),
                torch.empty(2, 24, 16, 3, dtype=torch.uint8, device=DEV).transpose(1, 2),
                torch.empty(2, 16, 24, 3, dtype=torch.uint8)):
        with pytest.raises(ValueError):
            render.overlay_frames(frames, _K(16, 24), [m], out=bad)
    good = torch.empty_like(frames)
    assert render.overlay_frames(frames, _K(16, 24), [m], out=good) is good
