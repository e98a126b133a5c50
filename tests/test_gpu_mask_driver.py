"""GPU: the batched mask-driven folder driver (process_batch_manopara_with_mask(batched=True), hamer_yolo_amd/mask_boxes.py)
against the reference's loop (batched=False) on a folder of six 480 x 640 frames: a normal mask, a missing mask file, a mask
without label 3, a single-pixel label, an int64 mask, a mask with labels 3 and 4; an intrinsics directory that lacks one frame's
txt.  On the precise route a hand's bytes do not depend on its batch, so betas and cam_t are the loop's bits; on the default
route the batch size picks the GEMM tile and the tolerances are those of the chunked-driver tests.  Also left_label, the
--masks command line, and a round trip through --hand-maps' masks."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from hamer_yolo_amd import infer, render, synth  # noqa: E402
from hamer_yolo_amd.infer import hamer_inference, process_batch_manopara, process_batch_manopara_with_mask  # noqa: E402
from hamer_yolo_amd.mask_boxes import MaskBoxes  # noqa: E402

H, W = 480, 640
K0 = np.array([[600.0, 0, 320], [0, 610.0, 240], [0, 0, 1]], np.float32)


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
    return hamer_inference(_Cfg)


@pytest.fixture(scope="module")
def hi_precise():
    return hamer_inference(_Cfg, precise=True)


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    from PIL import Image
    root = tmp_path_factory.mktemp("maskjob")
    rgb, masks, ks = root / "rgb", root / "masks", root / "k"
    for d in (rgb, masks, ks):
        d.mkdir()
    for i in range(6):
        Image.fromarray(synth.frame_u8(H, W, seed=130 + i).numpy()[:, :, ::-1]).save(rgb / f"f{i}.bmp")
        m = np.zeros((H, W), np.int64 if i == 4 else np.uint8)
        if i in (0, 4, 5):
            m[150 + 10 * i:281 + 10 * i, 200 - 20 * i:331 - 20 * i] = 3
        if i == 2:
            m[100:200, 100:200] = 2                               # no label 3
        if i == 3:
            m[77, 501] = 3                                        # a single pixel: a label whose box has no area
        if i == 4:
            m[0, 0] = 3 + 256                                     # fits no byte: no label
        if i == 5:
            m[300:420, 400:520] = 4
        if i != 1:                                                # f1: no mask file
            np.save(masks / f"f{i}.npy", m)
        if i != 4:                                                # f4: no intrinsics of its own
            np.savetxt(ks / f"f{i}.txt", K0 + np.float32(i))
    return {"root": root, "rgb": str(rgb), "masks": str(masks), "k": str(ks)}


def _records(path):
    return {f: np.load(os.path.join(path, f), allow_pickle=True).item() for f in sorted(os.listdir(path))}


def _both(folder, model, tag):
    """(records of the loop, records of the batched driver, the batched driver's stats), once per model."""
    cache = folder.setdefault("runs", {})
    if tag not in cache:
        loop, batched = str(folder["root"] / f"loop_{tag}"), str(folder["root"] / f"batched_{tag}")
        assert process_batch_manopara_with_mask(folder["rgb"], folder["masks"], loop, folder["k"], hamer=model) is None
        st = process_batch_manopara_with_mask(folder["rgb"], folder["masks"], batched, folder["k"], hamer=model, batched=True)
        cache[tag] = (_records(loop), _records(batched), st)
    return cache[tag]


def _same_files(a, b):
    assert sorted(a) == sorted(b) == ["f0.npy", "f3.npy", "f4.npy", "f5.npy"]
    assert a["f3.npy"] == b["f3.npy"] == {"left": None, "right": None}               # the label exists, the estimate had no crop
    for f in ("f0.npy", "f4.npy", "f5.npy"):
        assert a[f]["left"] is None and b[f]["left"] is None
        assert a[f]["right"]["is_right"] is True and b[f]["right"]["is_right"] is True
        assert set(a[f]["right"]) == set(b[f]["right"])


def test_precise_route_is_the_loop_bit_for_bit(folder, hi_precise):
    loop, batched, st = _both(folder, hi_precise, "precise")
    _same_files(loop, batched)
    assert st["images"] == 6 and st["hands"] == 3 and st["files"] == 4 and st["det_passes"] == 1
    assert sorted(st["forward_sizes"]) == [1, 2]                # the frame without a K went through a camera step of its own
    for f in ("f0.npy", "f4.npy", "f5.npy"):
        a, b = loop[f]["right"], batched[f]["right"]
        for key in ("betas", "cam_t"):
            assert a[key].dtype == b[key].dtype == np.float32 and a[key].shape == b[key].shape
            np.testing.assert_array_equal(a[key].view(np.uint32), b[key].view(np.uint32), err_msg=f"{f} {key}")
        for key in ("theta", "pose_hand", "pose_global"):       # (the two drivers convert rotations on the host with different code)
            np.testing.assert_allclose(b[key], a[key], rtol=0, atol=1e-6, err_msg=f"{f} {key}")


def test_default_route_matches_the_loop(folder, hi):
    loop, batched, st = _both(folder, hi, "default")
    _same_files(loop, batched)
    assert st["hands"] == 3 and st["files"] == 4
    for f in ("f0.npy", "f4.npy", "f5.npy"):
        for key in ("betas", "theta", "cam_t", "pose_hand", "pose_global"):
            np.testing.assert_allclose(batched[f]["right"][key], loop[f]["right"][key], rtol=1e-4, atol=2e-4, err_msg=f"{f} {key}")


def test_left_label_adds_the_left_record_of_the_sixth_frame_only(folder, hi):
    _, base, _ = _both(folder, hi, "default")
    out = str(folder["root"] / "left")
    st = process_batch_manopara_with_mask(folder["rgb"], folder["masks"], out, folder["k"], hamer=hi, batched=True, left_label=4)
    got = _records(out)
    assert sorted(got) == sorted(base) and st["hands"] == 4
    for f in got:
        assert (got[f]["left"] is not None) == (f == "f5.npy"), f
        if base[f]["right"] is not None:
            for key in ("betas", "theta", "cam_t"):
                np.testing.assert_allclose(got[f]["right"][key], base[f]["right"][key], rtol=1e-4, atol=2e-4, err_msg=f"{f} {key}")
    left = got["f5.npy"]["left"]
    assert left["is_right"] is False
    ref, _ = hi.estimate_from_rgb(synth.frame_u8(H, W, seed=135).numpy(), [["left", [400.0, 300.0, 519.0, 419.0]]], K0 + np.float32(5))
    want = infer.hand_record(ref, False, 0)
    for key in ("betas", "theta", "cam_t"):
        np.testing.assert_allclose(left[key], want[key], rtol=1e-4, atol=2e-4, err_msg=key)


def test_masks_command_line_writes_the_python_calls_files(folder, hi, monkeypatch):
    _, base, _ = _both(folder, hi, "default")
    out, obj = str(folder["root"] / "cli"), str(folder["root"] / "cli_obj")
    monkeypatch.setattr(infer, "hamer_inference", lambda cfg: hi)
    infer.main(["--input", folder["rgb"], "--output", out, "--masks", folder["masks"], "--intrinsics", folder["k"], "--obj", obj])
    got = _records(out)
    assert sorted(got) == sorted(base)
    for f in got:
        assert (got[f]["right"] is None) == (base[f]["right"] is None) and got[f]["left"] is None
        if got[f]["right"] is not None:
            for key in ("betas", "theta", "cam_t"):             # (the same hands in the same forwards; run-to-run within the route's tolerance)
                np.testing.assert_allclose(got[f]["right"][key], base[f]["right"][key], rtol=1e-4, atol=2e-4, err_msg=f"{f} {key}")
    assert sorted(os.listdir(obj)) == ["f0.obj", "f4.obj", "f5.obj"]
    out2 = str(folder["root"] / "cli_label")
    infer.main(["--input", folder["rgb"], "--output", out2, "--masks", folder["masks"], "--mask-label", "4", "--left-mask-label", "2"])
    got2 = _records(out2)
    assert sorted(got2) == ["f2.npy", "f5.npy"] and got2["f2.npy"]["right"] is None and got2["f2.npy"]["left"]["is_right"] is False
    assert got2["f5.npy"]["right"]["is_right"] is True and got2["f5.npy"]["left"] is None
    with pytest.raises(SystemExit):
        infer.main(["--input", folder["rgb"], "--output", out2, "--masks", folder["masks"], "--precise-detector"])


def test_round_trip_through_hand_maps(hi, tmp_path):
    """process_batch_manopara with given boxes -> --hand-maps' masks -> the batched mask driver: a record per frame, from the
    tight box of the written mask."""
    from PIL import Image
    rgb, npy, maps, rec = (tmp_path / d for d in ("rgb", "npy", "maps", "rec"))
    rgb.mkdir()
    for i in range(2):
        Image.fromarray(synth.frame_u8(240, 320, seed=60 + i).numpy()[:, :, ::-1]).save(rgb / f"g{i}.png")
    process_batch_manopara(str(rgb), str(npy), None, hamer=hi, detector=_FixedDetector([["right", [60.0, 50.0, 120.0, 120.0]]]))
    assert render.hand_maps_folder(str(rgb), str(npy), str(maps), hi, label=3) == 2
    st = process_batch_manopara_with_mask(str(rgb), str(maps), str(rec), hamer=hi, batched=True)
    assert sorted(os.listdir(rec)) == ["g0.npy", "g1.npy"] and st["hands"] == 2 and st["frames"] == 2
    paths = infer._list_images(str(rgb))
    seen = {os.path.basename(p): dets for p, dets, _ in infer.iter_folder_results(paths, hi, MaskBoxes(str(maps)))}
    loop = tmp_path / "loop"
    process_batch_manopara_with_mask(str(rgb), str(maps), str(loop), hamer=hi)
    for i in range(2):
        rows, cols = np.nonzero(np.load(maps / f"g{i}.npy") == 3)
        assert len(rows) > 0
        box = [float(cols.min()), float(rows.min()), float(cols.max()), float(rows.max())]
        assert seen[f"g{i}.png"] == [["right", box]] == [["right", infer.get_bbox_from_npy(str(maps / f"g{i}.npy"))]]
        got = np.load(rec / f"g{i}.npy", allow_pickle=True).item()
        want = np.load(loop / f"g{i}.npy", allow_pickle=True).item()
        assert got["left"] is None and got["right"]["is_right"] is True
        for key in ("betas", "theta", "cam_t"):
            np.testing.assert_allclose(got["right"][key], want["right"][key], rtol=1e-4, atol=2e-4, err_msg=f"g{i} {key}")
    render.release_workspaces()
