"""Host checks of the mask boxes (hm_mask_boxes, hamer_yolo_amd.mask_boxes.MaskBoxes, the batched
process_batch_manopara_with_mask): the numpy rule of tests/mask_boxes_rule.py against get_bbox_from_npy; the labels MaskBoxes
accepts and the queries it asks; the surface and every argument refusal of the C entry point, without a device; the new parser
options; and, with stub models on the host-only path of the folder pipeline, the pairing of files, masks and intrinsics -- hands
of frames with a K and hands of frames without one never share a camera step.  The box step is injected there: the library has
no CPU form of it.  No GPU."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mask_boxes_rule as BR  # noqa: E402
from test_folder_pipeline import _rz, _write_bmp  # noqa: E402

from hamer_yolo_amd import build as B  # noqa: E402
from hamer_yolo_amd import infer  # noqa: E402
from hamer_yolo_amd import lib as L  # noqa: E402
from hamer_yolo_amd.hamer.utils import mask_eval as ME  # noqa: E402
from hamer_yolo_amd.mask_boxes import MaskBoxes, as_label_bytes  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ the rule
def _random_mask(H, W, seed, dtype):
    rng = np.random.default_rng(seed)
    if dtype == np.bool_:
        return rng.random((H, W)) < 0.01
    m = np.zeros((H, W), dtype)
    for label in (1, 3, 4):
        if rng.random() < 0.8:
            ys, xs = rng.integers(0, H, 12), rng.integers(0, W, 12)
            m[ys, xs] = label
    if np.dtype(dtype).itemsize > 1:
        m[rng.integers(0, H), rng.integers(0, W)] = 3 + 256          # does not fit a byte: no label
        if np.dtype(dtype).kind == "i":
            m[rng.integers(0, H), rng.integers(0, W)] = -253
    return m


@pytest.mark.parametrize("dtype", [np.uint8, np.int32, np.int64, np.bool_])
def test_rule_is_get_bbox_from_npy(tmp_path, dtype):
    seen = set()
    for seed in range(12):
        H, W = 20 + seed, 31 + 3 * seed
        m = _random_mask(H, W, 50 * seed + 7, dtype)
        path = str(tmp_path / f"m{seed}.npy")
        np.save(path, m)
        stored = as_label_bytes(np.load(path, allow_pickle=False))[None]
        assert stored.dtype == np.uint8 and stored.shape == (1, H, W)
        for label in (1, 3, 4, 7):
            want = infer.get_bbox_from_npy(path, target_val=label)
            row = BR.boxes(stored, [(0, label)])[0].tolist()
            seen.add(want is None)
            if want is None:
                assert row == list(BR.EMPTY)
            else:
                assert [float(v) for v in row[:4]] == want and all(isinstance(v, float) for v in want)
                assert row[4] == int((m == label).sum()) > 0
    assert seen == {True, False}                                    # labels present and absent were both met
    assert BR.boxes(np.zeros((2, 3, 3), np.uint8), [(-1, 0), (2, 0)]).tolist() == [list(BR.EMPTY)] * 2
    any_label = np.zeros((1, 5, 7), np.uint8)
    any_label[0, 1, 2], any_label[0, 4, 6] = 9, 200
    assert BR.boxes(any_label, [(0, -1)]).tolist() == [[2, 1, 6, 4, 2]]


def test_missing_mask_file_warns_as_get_bbox_from_npy(tmp_path, capsys):
    src = MaskBoxes(str(tmp_path))
    assert infer.get_bbox_from_npy(src.mask_path("/x/rgb/f7.png")) is None
    want = capsys.readouterr().out
    assert src._load("/x/rgb/f7.png", (4, 4)) is None
    assert capsys.readouterr().out == want and "mask not found" in want and "f7.npy" in want


# ------------------------------------------------------------------ MaskBoxes
@pytest.mark.parametrize("kw", [dict(right_label=-1), dict(right_label=256), dict(left_label=256), dict(left_label=-1),
                                dict(right_label=3.5), dict(right_label=None), dict(right_label=True)])
def test_maskboxes_rejects_labels_outside_a_byte(kw):
    with pytest.raises(ValueError):
        MaskBoxes("masks", **kw)


def test_query_list():
    assert MaskBoxes("m").sides == [("right", 3)] and MaskBoxes("m").wants_paths
    assert MaskBoxes("m").queries(3) == [(0, 3), (1, 3), (2, 3)]
    assert MaskBoxes("m", right_label=0, left_label=255).queries(2) == [(0, 0), (0, 255), (1, 0), (1, 255)]
    assert MaskBoxes("m", left_label=4).queries(2) == [(0, 3), (0, 4), (1, 3), (1, 4)] and MaskBoxes("m").queries(0) == []
    t = ME.box_query_table(MaskBoxes("m", left_label=4).queries(2))
    assert t.dtype == np.int32 and t.shape == (4, 2) and t.flags.c_contiguous and ME.box_query_table([]).shape == (0, 2)
    with pytest.raises(ValueError):
        ME.box_query_table([(2 ** 31, 3)])
    src = MaskBoxes("m", left_label=4)
    assert src._detections([[5, 6, 9, 8, 11], [-1, -1, -1, -1, 0]]) == ([["right", [5.0, 6.0, 9.0, 8.0]]], True)
    assert src._detections([[-1, -1, -1, -1, 0], [2, 2, 2, 2, 1]]) == ([["left", [2.0, 2.0, 2.0, 2.0]]], True)
    assert src._detections([[-1, -1, -1, -1, 0]] * 2) == ([], False)
    with pytest.raises(ValueError):
        src.detect_frames_enqueue([torch.zeros(4, 4, 3, dtype=torch.uint8)])          # the paths are what this source asks for


# ------------------------------------------------------------------ surface and refusals
def test_surface():
    header = open(os.path.join(ROOT, "include", "hamer_hip.h")).read()
    lib = L.load()
    assert re.search(r"\bint hm_mask_boxes\(", header) and "hm_mask_boxes" in L.EXPORTS and hasattr(lib, "hm_mask_boxes")
    assert "typedef struct hm_box_query { int32_t frame, label; } hm_box_query;" in header
    assert "mask_boxes.hip" in B.SOURCES and os.path.exists(os.path.join(B.CSRC, "mask_boxes.hip"))
    assert re.search(r"#define HM_VERSION 402\b", header) and L.HM_VERSION == 402 and lib.hm_version() == 402
    src = open(os.path.join(B.CSRC, "mask_boxes.hip")).read()
    assert "getenv" not in src and "hipMalloc" not in src and "asm" not in src
    assert "hipDeviceSynchronize" not in src and "hipStreamSynchronize" not in src and "float" not in src and "double" not in src
    assert C.sizeof(L.BoxQuery) == 8 and [f[0] for f in L.BoxQuery._fields_] == ["frame", "label"]


def _call(**kw):
    """hm_mask_boxes over MADE-UP device addresses that are never dereferenced: every case must fail (or, for Q == 0, succeed)
    in the host part, before any launch."""
    a = dict(mask=0x20000, N=2, H=37, W=53, queries=0x30000, Q=3, boxes=0x40000, stream=None)
    a.update(kw)
    lib = L.load()
    rc = lib.hm_mask_boxes(a["mask"], a["N"], a["H"], a["W"], a["queries"], a["Q"], a["boxes"], a["stream"])
    return rc, lib.hm_last_error_string().decode()


@pytest.mark.parametrize("kw,word", [
    (dict(mask=None), "null"), (dict(queries=None), "null"), (dict(boxes=None), "null"), (dict(N=0), "positive"),
    (dict(H=0), "positive"), (dict(W=0), "positive"), (dict(N=-1), "positive"), (dict(H=-5), "positive"),
    (dict(N=1024, H=1024, W=2048), "2^31"), (dict(N=2, H=32768, W=32768), "2^31"), (dict(Q=-1), "Q"),
    (dict(queries=0x30002), "aligned"), (dict(boxes=0x40001), "aligned"), (dict(mask=None, Q=0), "null"),
])
def test_argument_refusals_before_any_device_work(kw, word):
    rc, msg = _call(**kw)
    assert rc == -1 and word in msg and "hm_mask_boxes" in msg, (rc, msg)          # HM_ERR_ARG


def test_no_query_is_no_launch():
    assert _call(Q=0)[0] == 0 and _call(Q=0, queries=None, boxes=None)[0] == 0
    assert _call(Q=0, N=1, H=1, W=1)[0] == 0 and _call(Q=0, N=1, H=1, W=(1 << 31) - 1)[0] == 0


def test_wrapper_has_no_cpu_path():
    with pytest.raises(ValueError, match="no CPU path"):
        ME.mask_boxes(torch.zeros(1, 4, 4, dtype=torch.uint8), [(0, 3)])


# ------------------------------------------------------------------ the parser
def _parse(argv):
    ap = infer._parser()
    args = ap.parse_args(["--input", "rgb", "--output", "out"] + argv)
    infer.mask_args(ap, args)
    return args


def test_parser_options_and_mutual_exclusion(tmp_path, capsys):
    a = _parse([])
    assert a.masks is None and a.mask_label == 3 and a.left_mask_label is None
    a = _parse(["--masks", "m", "--mask-label", "5", "--left-mask-label", "6", "--intrinsics", str(tmp_path), "--precise-hamer",
                "--antialias-crop", "--obj", "o"])
    assert (a.masks, a.mask_label, a.left_mask_label, a.intrinsics) == ("m", 5, 6, str(tmp_path)) and a.precise_hamer and a.antialias_crop
    _parse(["--masks", "m", "--render", "r", "--render-style", "smooth", "--hand-maps", "h", "--intrinsics", "K.txt"])
    for bad in (["--masks", "m", "--yolo-weights", "synthetic:0"], ["--masks", "m", "--precise-detector"],
                ["--masks", "m", "--tta-detector"], ["--mask-label", "4"], ["--left-mask-label", "4"],
                ["--masks", "m", "--mask-label", "256"], ["--masks", "m", "--left-mask-label", "-1"],
                ["--masks", "m", "--intrinsics", str(tmp_path), "--render", "r"],
                ["--masks", "m", "--intrinsics", str(tmp_path), "--hand-maps", "h"]):
        with pytest.raises(SystemExit) as e:
            _parse(bad)
        assert e.value.code == 2, bad
    assert "no detector to act on" in capsys.readouterr().err


# ------------------------------------------------------------------ files, masks and intrinsics through the pipeline
H_, W_ = 24, 32


def _img(i):
    return np.random.default_rng(500 + i).integers(0, 256, (H_, W_, 3), dtype=np.uint8)


class RuleBoxes(MaskBoxes):
    """MaskBoxes with the device step replaced by the numpy rule (the injected box step); everything else is the class's own."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.calls, self.slots = [], []

    def _boxes_enqueue(self, masks, hw, dev, slots=None):
        self.slots.append(slots)
        stack = np.stack(masks)
        assert stack.dtype == np.uint8 and stack.shape[1:] == tuple(hw)
        self.calls.append(len(masks))
        return BR.boxes(stack, self.queries(len(masks))), None


class CameraHamer:
    """A stub model that records every camera step: which frames (by pixel mean), which boxes, and which K each hand got."""
    device = torch.device("cpu")

    def __init__(self):
        self.steps = []

    def estimate_from_frames(self, frames, dets_lists, k_real=None, depth_refine=None):
        rows = [(float(fr.numpy().astype(np.float64).mean()), label, box) for fr, dl in zip(frames, dets_lists) for label, box in dl]
        n = len(rows)
        if k_real is None:
            ks = [None] * n
        else:
            k = np.asarray(k_real, np.float32)
            assert k.shape in ((3, 3), (n, 3, 3)), k.shape
            ks = [k if k.ndim == 2 else k[i] for i in range(n)]
        self.steps.append([(r[0], r[1], tuple(r[2]), None if k is None else float(k[0, 0])) for r, k in zip(rows, ks)])
        fx = [0.0 if k is None else float(k[0, 0]) for k in ks]
        betas = torch.tensor([[r[0] + j for j in range(10)] for r in rows], dtype=torch.float32)
        go = torch.tensor(np.stack([_rz(0.01 * r[2][0] + 0.2)[None] for r in rows]))
        hp = torch.tensor(np.stack([np.stack([_rz(0.02 * (j + 1) + 0.003 * r[2][3]) for j in range(15)]) for r in rows]))
        return {"pred_mano_params": {"betas": betas, "global_orient": go, "hand_pose": hp},
                "pred_cam_t_full": torch.tensor([[r[2][0], r[2][1], f] for r, f in zip(rows, fx)], dtype=torch.float32),
                "do_flip": torch.tensor([0.0 if r[1] == 'right' else 1.0 for r in rows])}, None


@pytest.fixture()
def job(tmp_path):
    """Ten frames: masks with label 3 in eight of them (one as int64, one also with label 4, one a single pixel, one of another
    shape), none for f3, label 2 only in f5; a K for the even frames only."""
    rgb, masks, ks = tmp_path / "rgb", tmp_path / "masks", tmp_path / "k"
    for d in (rgb, masks, ks):
        d.mkdir()
    boxes = {}
    for i in range(10):
        _write_bmp(str(rgb / f"f{i}.bmp"), _img(i))
        if i == 3:
            continue
        m = np.zeros((H_, W_), np.int64 if i == 4 else np.uint8)
        if i == 5:
            m[2:5, 2:5] = 2
        elif i == 7:
            m[9, 11] = 3                                              # a single pixel: a label without a crop
        else:
            m[3 + i:9 + i, 2 * i:2 * i + 7] = 3
            boxes[i] = [float(2 * i), float(3 + i), float(2 * i + 6), float(8 + i)]
        if i == 6:
            m[1:4, 20:30] = 4
        if i == 8:                                                    # another shape than its frame: the host rule, alone
            m = np.zeros((H_ + 2, W_), np.uint8)
            m[5:9, 4:8] = 3
            boxes[i] = [4.0, 5.0, 7.0, 8.0]
        np.save(masks / f"f{i}.npy", m)
        if i % 2 == 0:
            np.savetxt(ks / f"f{i}.txt", np.array([[100.0 + i, 0, 16], [0, 100.0 + i, 12], [0, 0, 1]]))
    return str(rgb), str(masks), str(ks), boxes


def _run(job, monkeypatch, intrinsics, left_label=None, **kw):
    from hamer_yolo_amd import mask_boxes as MB
    rgb, masks, ks, boxes = job
    made = []

    def factory(*a, **k):
        made.append(RuleBoxes(*a, **k))
        return made[-1]
    monkeypatch.setattr(MB, "MaskBoxes", factory)
    ham = CameraHamer()
    out = os.path.join(os.path.dirname(rgb), f"out{len(os.listdir(os.path.dirname(rgb)))}")
    st = infer.process_batch_manopara_with_mask(rgb, masks, out, {"dir": ks, "none": None}.get(intrinsics, intrinsics), hamer=ham,
                                                batched=True, left_label=left_label, **kw)
    return out, st, ham, made[0]


@pytest.mark.parametrize("kw", [dict(), dict(hands_per_forward=3, frames_per_step=2, det_frames=4), dict(hands_per_forward=1, frames_per_step=1)])
def test_pairing_of_files_masks_and_intrinsics(job, monkeypatch, capsys, kw):
    out, st, ham, src = _run(job, monkeypatch, "dir", **kw)
    boxes = job[3]
    # files: every frame whose label exists, the single-pixel one with the empty record; none for f3 (no mask) and f5 (no label 3)
    assert sorted(os.listdir(out)) == [f"f{i}.npy" for i in (0, 1, 2, 4, 6, 7, 8, 9)] and st["files"] == 8 and st["hands"] == 7
    assert "mask not found" in capsys.readouterr().out
    assert np.load(os.path.join(out, "f7.npy"), allow_pickle=True).item() == {"left": None, "right": None}
    key = {float(_img(i).astype(np.float64).mean()): i for i in range(10)}
    seen = {}
    for step in ham.steps:
        # a camera step holds hands WITH a K, each with its own frame's, or hands WITHOUT one: never both
        assert len({k is None for _, _, _, k in step}) == 1, step
        for mean, label, box, k in step:
            i = key[mean]
            assert i not in seen and label == "right" and list(box) == boxes[i]
            assert k == (100.0 + i if i % 2 == 0 else None)
            seen[i] = k
    assert sorted(seen) == [0, 1, 2, 4, 6, 8, 9]
    for i in seen:
        rec = np.load(os.path.join(out, f"f{i}.npy"), allow_pickle=True).item()
        assert rec["left"] is None and rec["right"]["is_right"] is True
        np.testing.assert_array_equal(rec["right"]["cam_t"], np.float32([boxes[i][0], boxes[i][1], seen[i] or 0.0]))
        assert rec["right"]["betas"][0] == np.float32(_img(i).astype(np.float64).mean())
        assert rec["right"]["theta"].shape == (48,) and np.array_equal(rec["right"]["theta"][3:], rec["right"]["pose_hand"])
    # the batched call never saw the mask of another shape, nor the missing one
    assert sum(src.calls) == 8 and sorted(src.labelled) == sorted(os.path.join(job[0], f"f{i}.bmp") for i in (0, 1, 2, 4, 6, 7, 8, 9))


def test_masks_are_read_into_a_ring_next_to_each_other(job, monkeypatch, tmp_path):
    """The decode threads read every mask into the slot of its frame's place in the ring, so a pass's masks go up as one slice;
    the frames without a batched mask (f3: no file, f8: another shape) leave gaps no query names."""
    from hamer_yolo_amd.mask_boxes import read_bytes_into
    _, _, _, src = _run(job, monkeypatch, "dir")
    assert src.slots == [[0, 1, 2, 4, 5, 6, 7, 9]] and src._ring[:2] == ((H_, W_), 10) and src.queries([0, 2]) == [(0, 3), (2, 3)]
    _, _, _, src = _run(job, monkeypatch, "dir", frames_per_step=4, det_frames=4)
    assert src.slots == [[0, 1, 2], [4, 5, 6, 7], [9]]
    m = np.random.default_rng(3).integers(0, 256, (7, 9), dtype=np.uint8)
    for name, arr, ok in (("u8", m, True), ("i64", m.astype(np.int64), False), ("f", np.asfortranarray(m), False),
                          ("shape", m[:, :8], False), ("bool", m > 7, False)):
        np.save(tmp_path / f"{name}.npy", arr)
        dest = np.full((7, 9), 255, np.uint8)
        assert read_bytes_into(str(tmp_path / f"{name}.npy"), dest) is ok, name
        assert not ok or np.array_equal(dest, m)
    assert read_bytes_into(str(tmp_path / "none.npy"), np.zeros((7, 9), np.uint8)) is False
    (tmp_path / "short.npy").write_bytes((tmp_path / "u8.npy").read_bytes()[:-5])
    assert read_bytes_into(str(tmp_path / "short.npy"), np.zeros((7, 9), np.uint8)) is False


def test_fixed_and_default_camera_keep_the_single_matrix_path(job, monkeypatch):
    K = np.array([[77.0, 0, 16], [0, 77.0, 12], [0, 0, 1]], np.float32)
    kfile = os.path.join(os.path.dirname(job[0]), "K.txt")
    np.savetxt(kfile, K)
    out, st, ham, _ = _run(job, monkeypatch, kfile, hands_per_forward=4)
    assert [len(s) for s in ham.steps] == st["forward_sizes"] and sum(st["forward_sizes"]) == 7
    assert all(k == 77.0 for step in ham.steps for _, _, _, k in step)
    out2, st2, ham2, _ = _run(job, monkeypatch, "none", hands_per_forward=4)
    assert all(k is None for step in ham2.steps for _, _, _, k in step) and st2["forward_sizes"] == st["forward_sizes"]
    assert sorted(os.listdir(out)) == sorted(os.listdir(out2))


def test_left_label_and_sharding(job, monkeypatch):
    out, st, ham, src = _run(job, monkeypatch, "dir", left_label=4)
    assert src.queries(1) == [(0, 3), (0, 4)] and st["hands"] == 8
    for i in (0, 1, 2, 4, 6, 7, 8, 9):
        rec = np.load(os.path.join(out, f"f{i}.npy"), allow_pickle=True).item()
        assert (rec["left"] is not None) == (i == 6)
    rec = np.load(os.path.join(out, "f6.npy"), allow_pickle=True).item()
    assert rec["left"]["is_right"] is False and rec["left"]["cam_t"].tolist() == [20.0, 1.0, 106.0]
    names = []
    for r in range(3):
        o, s, _, _ = _run(job, monkeypatch, "dir", rank=r, world=3)
        assert s["images"] == len(infer.shard_paths(list(range(10)), r, 3))
        names += os.listdir(o)
    assert sorted(names) == sorted(os.listdir(out))                   # the ranks' files partition the single run's


def test_the_loop_is_untouched_by_the_new_arguments(job):
    import inspect
    p = inspect.signature(infer.process_batch_manopara_with_mask).parameters
    assert list(p)[:9] == ["input_folder", "mask_folder", "output_folder", "intrinsics_path", "hamer", "batched", "left_label", "rank", "world"]
    assert p["batched"].default is False and p["left_label"].default is None and p["intrinsics_path"].default is None
    with pytest.raises(ValueError):
        infer.process_batch_manopara_with_mask(job[0], job[1], "unused", left_label=4)
