"""CPU tests of how the folder overlay paths stream: frames grouped by the size in their headers, cut into passes, decoded
one pass at a time, and at most PASSES_IN_FLIGHT passes of encodes pending.  The GPU steps are replaced by stand-ins here;
tests/test_gpu_render.py runs the real ones."""
import os
from concurrent.futures import ThreadPoolExecutor
from types import SimpleNamespace

import numpy as np
import torch
from PIL import Image

from hamer_yolo_amd import infer, render


def test_frame_size_reads_the_header(tmp_path):
    Image.fromarray(np.zeros((37, 53, 3), np.uint8)).save(tmp_path / "a.png")
    Image.fromarray(np.zeros((21, 10, 3), np.uint8)).save(tmp_path / "b.bmp")
    (tmp_path / "c.png").write_bytes(b"not an image")
    assert render.frame_size(str(tmp_path / "a.png")) == (37, 53)
    assert render.frame_size(str(tmp_path / "b.bmp")) == (21, 10)
    assert render.frame_size(str(tmp_path / "c.png")) is None
    assert render.frame_size(str(tmp_path / "missing.png")) is None


def test_size_passes_groups_and_cuts():
    sizes = [(4, 6), (8, 8), (4, 6), None, (4, 6), (8, 8), (4, 6), (4, 6)]
    assert render.size_passes(sizes, 2) == [((4, 6), [0, 2]), ((4, 6), [4, 6]), ((4, 6), [7]), ((8, 8), [1, 5])]
    assert render.size_passes(sizes, 16) == [((4, 6), [0, 2, 4, 6, 7]), ((8, 8), [1, 5])]
    assert render.size_passes([], 4) == []


def test_pass_writer_keeps_few_passes_pending(monkeypatch, tmp_path):
    saved = []
    monkeypatch.setattr(render, "_save", lambda p, img: saved.append(p))
    with ThreadPoolExecutor(4) as pool:
        w = render.PassWriter(pool, in_flight=2)
        for k in range(6):
            w.submit([(f"p{k}_{j}", None) for j in range(3)])
            assert len(w.pending) <= 2
            assert {f"p{i}_{j}" for i in range(k - 1) for j in range(3)} <= set(saved)     # older passes are finished
        assert w.close() == 18 and len(saved) == 18 and not w.pending


def _folder(tmp_path, n, shapes):
    img, npy = tmp_path / "rgb", tmp_path / "npy"
    img.mkdir(); npy.mkdir()
    for i in range(n):
        h, w = shapes[i % len(shapes)]
        Image.fromarray(np.full((h, w, 3), i, np.uint8)).save(img / f"f{i:03d}.png")
        hand = {"betas": np.zeros(10, np.float32), "pose_global": np.zeros(3, np.float32), "pose_hand": np.zeros(45, np.float32),
                "cam_t": np.array([0, 0, 1], np.float32), "is_right": True}
        np.save(npy / f"f{i:03d}.npy", {"right": hand, "left": None})
    return str(img), str(npy)


def test_render_folder_decodes_one_pass_at_a_time(monkeypatch, tmp_path):
    """11 frames of two sizes, passes of 3: every overlay call sees only its own pass decoded, and every file is written
    with its own frame's bytes."""
    img, npy = _folder(tmp_path, 11, [(12, 16), (20, 8)])
    decoded, calls = [], []
    real_read = infer._imread_bgr

    def read(path, *a, **k):
        decoded.append(path)
        return real_read(path)

    def fake_overlay(frames, K, meshes, style="flat"):
        calls.append((len(decoded), frames.shape[0], K[0, 2], K[1, 2]))
        assert len(meshes) == frames.shape[0]
        return frames
    monkeypatch.setattr(infer, "_imread_bgr", read)
    monkeypatch.setattr(render, "overlay_frames", fake_overlay)
    monkeypatch.setattr(render, "camera_vertices", lambda hamer, hands: torch.zeros(len(hands), 4, 3))
    hamer = SimpleNamespace(device=torch.device("cpu"), mano=SimpleNamespace(faces=np.zeros((2, 3), np.int32)),
                            cfg=SimpleNamespace(EXTRA=SimpleNamespace(FOCAL_LENGTH=5000.0), MODEL=SimpleNamespace(IMAGE_SIZE=256)))
    out = tmp_path / "out"
    assert render.render_folder(img, npy, str(out), hamer, ext=".png", frames_per_pass=3) == 11
    # sizes (12,16) x 6 frames -> passes 3, 3; (20,8) x 5 -> 3, 2; decoded count at each call = frames of passes so far
    assert [(d, n) for d, n, _, _ in calls] == [(3, 3), (6, 3), (9, 3), (11, 2)]
    assert [(cx, cy) for _, _, cx, cy in calls] == [(8.0, 6.0)] * 2 + [(4.0, 10.0)] * 2        # default camera: (W/2, H/2)
    for i in range(11):
        got = np.asarray(Image.open(out / f"f{i:03d}.png"))
        assert got.shape[:2] == [(12, 16), (20, 8)][i % 2] and (got == i).all()
    assert render._ws == {}
