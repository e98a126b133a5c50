"""Host checks of the mask scores (hm_mask_score, hamer.utils.mask_eval, hamer_yolo_amd.evaluate_masks): the numpy rule of
tests/mask_eval_rule.py against scipy's binary dilation and Euclidean distance transform and against the assign-then-patch form
of the boundary map; J, F, precision and recall from counts; the radius; and the surface -- exports, header, build list,
argument checks, the driver's parser.  No GPU."""
import ctypes as C
import inspect
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mask_eval_rule as MR  # noqa: E402

from hamer_yolo_amd import build as B  # noqa: E402
from hamer_yolo_amd import lib as L  # noqa: E402
from hamer_yolo_amd.hamer.utils import mask_eval as ME  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(37, 53, 1), (37, 53, 3), (64, 64, 2), (70, 131, 5), (9, 200, 4), (1, 17, 2), (23, 1, 2)]


def _pair(H, W, seed):
    return MR.blobs(H, W, seed), MR.blobs(H, W, seed + 100)


# ------------------------------------------------------------------ the rule
@pytest.mark.parametrize("H,W,r", SHAPES)
def test_rule_against_scipy(H, W, r):
    ndi = pytest.importorskip("scipy.ndimage")
    yy, xx = np.mgrid[-r:r + 1, -r:r + 1]
    disk = xx * xx + yy * yy <= r * r
    for seed in (1, 2, 3):
        pred, gt = _pair(H, W, seed)
        bp, bg = MR.bmap(pred), MR.bmap(gt)
        c = MR.counts(pred, gt, r)
        assert c[7] == H * W and c[0] == (pred & gt).sum() and c[1] == pred.sum() and c[2] == gt.sum()
        assert c[3] == bp.sum() and c[4] == bg.sum()
        for mine, other, k in ((bp, bg, 5), (bg, bp, 6)):
            by_dilation = (mine & ndi.binary_dilation(other, structure=disk)).sum()
            # distance_transform_edt: the distance to the nearest zero, so the other boundary is passed inverted
            near = ndi.distance_transform_edt(~other) ** 2 <= r * r + 1e-9 if other.any() else np.zeros_like(other)
            assert c[k] == by_dilation == (mine & near).sum(), (seed, k)


@pytest.mark.parametrize("H,W,r", SHAPES + [(2, 2, 0), (5, 7, 0)])
def test_boundary_map_equals_assign_then_patch(H, W, r):
    for seed in (1, 2, 3):
        s = MR.blobs(H, W, seed)
        b = MR.bmap(s)
        assert np.array_equal(b, MR.bmap_assign_then_patch(s)) and not b[-1, -1]
    for s in (np.zeros((H, W), bool), np.ones((H, W), bool)):
        assert not MR.bmap(s).any() and not MR.bmap_assign_then_patch(s).any()
    chk = (np.indices((H, W)).sum(0) % 2).astype(bool)
    assert np.array_equal(MR.bmap(chk), MR.bmap_assign_then_patch(chk))


def test_rule_hand_made():
    # a 2 x 2 square in a 5 x 6 image: the boundary is the 3 x 3 block up and left of its far corner, less that corner's own cell
    s = np.zeros((5, 6), bool)
    s[2:4, 2:4] = True
    b = MR.bmap(s)
    want = np.zeros_like(s)
    want[1:4, 1:4] = True
    want[2, 2] = False                                                    # its east, south and south-east are all inside
    assert np.array_equal(b, want)
    # two single pixels at offset (3, 4): distance 5
    p, g = np.zeros((20, 20), bool), np.zeros((20, 20), bool)
    p[5, 5] = True
    g[8, 9] = True
    assert MR.bmap(p).sum() == 4
    assert MR.counts(p, g, 4)[5] < 4 and MR.counts(p, g, 5)[5:7].tolist() == [4, 4]
    far = np.zeros((20, 20), bool)
    far[19, 19] = True                                                    # the bottom-right pixel: boundary at its three neighbours
    assert MR.bmap(far).sum() == 3 and not MR.bmap(far)[19, 19]
    assert MR.dilate(p, 0).sum() == 1 and MR.dilate(p, 1).sum() == 5 and MR.dilate(p, 2).sum() == 13


# ------------------------------------------------------------------ from counts
def test_jf_from_counts_cases():
    rows = np.array([
        [0, 0, 0, 0, 0, 0, 0, 100],          # both empty: J = 1, P = R = 1, F = 1
        [0, 0, 9, 0, 12, 0, 0, 100],         # only gt: J = 0, P = 1, R = 0, F = 0
        [0, 9, 0, 12, 0, 0, 0, 100],         # only pred: J = 0, P = 0, R = 1, F = 0
        [30, 100, 30, 0, 20, 0, 0, 100],     # a full pred (no boundary) against a blob
        [6, 10, 8, 7, 9, 3, 6, 100],         # the general case
        [5, 10, 8, 7, 9, 0, 0, 100],         # boundaries, none matched: P + R = 0, F = 0
    ], np.int64)
    got = ME.jf_from_counts(rows)
    assert set(got) == {"J", "F", "precision", "recall"} and all(v.dtype == np.float64 and v.shape == (6,) for v in got.values())
    assert got["J"].tolist() == [1.0, 0.0, 0.0, 0.3, 6 / 12, 5 / 13]
    assert got["precision"].tolist() == [1.0, 1.0, 0.0, 1.0, 3 / 7, 0.0]
    assert got["recall"].tolist() == [1.0, 0.0, 1.0, 0.0, 6 / 9, 0.0]
    p, r = 3 / 7, 6 / 9
    assert got["F"].tolist() == [1.0, 0.0, 0.0, 0.0, 2 * p * r / (p + r), 0.0]
    for i, row in enumerate(rows):
        assert MR.jf(row) == tuple(got[k][i] for k in ("J", "F", "precision", "recall"))
    empty = ME.jf_from_counts(np.zeros((0, 8), np.int64))
    assert all(v.shape == (0,) for v in empty.values())
    assert ME.jf_from_counts(torch.from_numpy(rows))["J"].tolist() == got["J"].tolist()


def test_bound_radius():
    assert ME.bound_radius(1080, 1920) == 18 and ME.bound_radius(720, 1280) == 12 and ME.bound_radius(37, 53) == 1
    assert ME.bound_radius(1080, 1920, bound_th=5) == 5 and ME.bound_radius(10, 10, 1) == 1
    assert ME.bound_radius(1080, 1920, 0.008) == int(np.ceil(0.008 * np.linalg.norm([1080, 1920])))
    p = inspect.signature(ME.bound_radius).parameters
    assert list(p) == ["H", "W", "bound_th"] and p["bound_th"].default == 0.008


# ------------------------------------------------------------------ surface
NAMES = ("hm_mask_score_workspace_bytes", "hm_mask_score")


def test_surface():
    header = open(os.path.join(ROOT, "include", "hamer_hip.h")).read()
    lib = L.load()
    for name in NAMES:
        assert re.search(r"\b%s\(" % name, header) and name in L.EXPORTS and hasattr(lib, name), name
    assert "typedef struct hm_mask_query" in header and "UNPINNED against DAVIS" in header
    assert "mask_eval.hip" in B.SOURCES and os.path.exists(os.path.join(B.CSRC, "mask_eval.hip"))
    assert re.search(r"#define HM_VERSION 402\b", header) and L.HM_VERSION == 402 and lib.hm_version() == 402
    src = open(os.path.join(B.CSRC, "mask_eval.hip")).read()
    assert "getenv" not in src and "hipMalloc" not in src and "asm" not in src
    assert "hipDeviceSynchronize" not in src and "hipStreamSynchronize" not in src and "float" not in src and "double" not in src
    assert C.sizeof(L.MaskQuery) == 16 and [f[0] for f in L.MaskQuery._fields_] == ["frame", "id_lo", "id_hi", "label"]
    assert lib.hm_mask_score_workspace_bytes.restype is C.c_size_t


def test_workspace_bytes():
    lib = L.load()
    prev = 0
    for Q in (1, 2, 3, 16, 64, 256):
        n = lib.hm_mask_score_workspace_bytes(Q, 1080, 1920, 18)
        assert n > prev and n % 8 == 0
        prev = n
    assert lib.hm_mask_score_workspace_bytes(0, 1080, 1920, 18) > 0
    assert lib.hm_mask_score_workspace_bytes(1, 1, 1, 0) > 0
    assert lib.hm_mask_score_workspace_bytes(1, 1080, 1920, 18) >= 2 * 1080 * 1920 // 8      # a bit per pixel and side at least
    assert lib.hm_mask_score_workspace_bytes(4, 70, 131, 5) == lib.hm_mask_score_workspace_bytes(4, 70, 131, 64)
    for bad in ((-1, 10, 10, 1), (1, 0, 10, 1), (1, 10, 0, 1), (1, 10, 10, -1), (1, 10, 10, 65)):
        assert lib.hm_mask_score_workspace_bytes(*bad) == 0, bad


def _call(**kw):
    """hm_mask_score over MADE-UP device addresses that are never dereferenced: every case below must fail in the host part,
    before any launch (on a machine with a GPU a regressed check would launch over these wild pointers)."""
    a = dict(pred_id=0x10000, mask=0x20000, N=2, H=37, W=53, queries=0x30000, Q=3, radius=3, counts=0x40000, workspace=0x50000,
             workspace_bytes=None, stream=None)
    a.update(kw)
    lib = L.load()
    if a["workspace_bytes"] is None:
        a["workspace_bytes"] = max(int(lib.hm_mask_score_workspace_bytes(max(a["Q"], 0), max(a["H"], 1), max(a["W"], 1), 3)), 8)
    rc = lib.hm_mask_score(a["pred_id"], a["mask"], a["N"], a["H"], a["W"], a["queries"], a["Q"], a["radius"], a["counts"],
                           a["workspace"], a["workspace_bytes"], a["stream"])
    return rc, lib.hm_last_error_string().decode()


@pytest.mark.parametrize("kw,word", [
    (dict(pred_id=None), "null"), (dict(mask=None), "null"), (dict(queries=None), "null"), (dict(counts=None), "null"),
    (dict(workspace=None), "null"), (dict(N=0), "positive"), (dict(H=0), "positive"), (dict(W=0), "positive"), (dict(N=-1), "positive"),
    (dict(N=1024, H=1024, W=2048), "2^31"), (dict(N=2, H=32768, W=32768), "2^31"), (dict(radius=-1), "radius"),
    (dict(radius=65), "radius"), (dict(Q=-1), "Q"), (dict(workspace_bytes=8), "workspace"),
    (dict(workspace_bytes=3 * 2 * 37 * 8 - 1), "workspace"), (dict(counts=0x40004), "aligned"), (dict(workspace=0x50004), "aligned"),
    (dict(pred_id=0x10002), "aligned"),
])
def test_argument_checks(kw, word):
    rc, msg = _call(**kw)
    assert rc == -1 and "hm_mask_score" in msg and word in msg, (rc, msg)          # HM_ERR_ARG


def test_exact_workspace_and_no_queries_pass_the_checks_without_a_launch():
    # Q == 0 returns before anything is read or launched, also with the other pointers NULL
    assert _call(Q=0)[0] == 0 and _call(Q=0, queries=None, counts=None, workspace=None, workspace_bytes=0)[0] == 0
    assert L.load().hm_mask_score_workspace_bytes(3, 37, 53, 3) == 3 * 2 * 37 * 8


# ------------------------------------------------------------------ the Python layer and the driver
def test_mask_counts_raises_on_host_tensors_and_bad_inputs():
    pid, m = torch.zeros(2, 8, 9, dtype=torch.int32), torch.zeros(2, 8, 9, dtype=torch.uint8)
    with pytest.raises(ValueError, match="GPU"):
        ME.mask_counts(pid, m, [(0, 0, 1, 3)])
    with pytest.raises(ValueError):
        ME.mask_counts(pid.numpy(), m.numpy(), [(0, 0, 1, 3)])
    p = inspect.signature(ME.mask_counts).parameters
    assert list(p) == ["pred_id", "mask", "queries", "radius", "bound_th", "counts"]
    assert p["radius"].default is None and p["bound_th"].default == 0.008 and p["counts"].default is None
    with pytest.raises(ValueError, match="frame 2"):
        ME._query_table([(0, 0, 1, 3), (2, 0, 1, 3)], 2)
    with pytest.raises(ValueError, match="frame -1"):
        ME._query_table([(-1, 0, 1, 3)], 2)
    t = ME._query_table([(1, 0, 2, 3), (0, 5, 5, -1)], 2)
    assert t.dtype == np.int32 and t.tolist() == [[1, 0, 2, 3], [0, 5, 5, -1]] and ME._query_table([], 2).shape == (0, 4)
    assert ME.COUNT_NAMES == MR.COUNT_NAMES


def test_evaluator_needs_no_gpu_until_called():
    ev = ME.MaskEvaluator()
    assert ev.n == 0 and ev.counts().shape == (0, 8) and all(v.shape == (0,) for v in ev.per_query().values())
    with pytest.raises(ValueError):
        ev.result()
    c = inspect.signature(ME.MaskEvaluator.__call__).parameters
    assert list(c)[:5] == ["self", "pred_id", "mask", "queries", "sync"] and c["sync"].default is False


def test_driver_parser_and_defaults():
    from hamer_yolo_amd import evaluate_masks as EM
    a = EM._parser().parse_args(["--pred", "A", "--images", "B", "--masks", "C"])
    assert (a.pred, a.images, a.masks, a.label, a.bound_th, a.intrinsics, a.json) == ("A", "B", "C", 3, 0.008, None, None)
    a = EM._parser().parse_args(["--pred", "A", "--images", "B", "--masks", "C", "--label", "5", "--bound-th", "12",
                                 "--intrinsics", "K.txt", "--json", "o.json"])
    assert (a.label, a.bound_th, a.intrinsics, a.json) == (5, 12.0, "K.txt", "o.json")
    with pytest.raises(SystemExit):
        EM._parser().parse_args(["--pred", "A"])
    p = inspect.signature(EM.score_folder).parameters
    assert list(p) == ["image_folder", "npy_folder", "mask_folder", "hamer", "k_real", "label", "bound_th", "rank", "world",
                       "frames_per_pass"]
    assert (p["k_real"].default, p["label"].default, p["bound_th"].default, p["rank"].default, p["world"].default,
            p["frames_per_pass"].default) == (None, 3, 0.008, 0, 1, 16)
    line = EM.format_line({"n": 4, "j_mean": 0.75, "j_recall": 1.0, "f_mean": 0.5, "f_recall": 0.25, "jf_mean": 0.625, "label": 3,
                           "bound_th": 0.008, "n_skipped": 2})
    assert all(w in line for w in ("4 frames", "J mean 0.7500", "F mean 0.5000", "J&F 0.6250", "skipped 2"))


def test_driver_mask_loading(tmp_path):
    from hamer_yolo_amd import evaluate_masks as EM
    m = np.zeros((6, 7), np.uint8)
    m[2:4, 3:5] = 3
    np.save(tmp_path / "a.npy", m)
    np.save(tmp_path / "wide.npy", m.astype(np.int32) * 100)
    np.save(tmp_path / "f.npy", m.astype(np.float32))
    got = EM._load_mask(str(tmp_path / "a.npy"), (6, 7))
    assert got.dtype == np.uint8 and np.array_equal(got, m)
    assert EM._load_mask(str(tmp_path / "a.npy"), (7, 6)) is None and EM._load_mask(str(tmp_path / "none.npy"), (6, 7)) is None
    assert EM._load_mask(str(tmp_path / "f.npy"), (6, 7)) is None
    assert not EM._load_mask(str(tmp_path / "wide.npy"), (6, 7)).any()                     # 300 is no byte label: dropped, not wrapped


def test_hamer_utils_still_exports_what_it_did():
    import hamer_yolo_amd.hamer.utils as U
    assert U.__all__ == ["eval_pose", "Evaluator"]
    from hamer_yolo_amd.hamer.utils import mask_eval
    assert mask_eval is ME and all(hasattr(ME, n) for n in ("bound_radius", "mask_counts", "jf_from_counts", "MaskEvaluator"))
