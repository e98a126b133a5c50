"""GPU: hm_mask_score against the numpy rule of tests/mask_eval_rule.py at the shapes where tiling, halos and bit packing can go
wrong, its batch / query invariance, buffers and determinism; hamer.utils.mask_eval; evaluate_masks.score_folder end to end on
a synthetic MANO model.

Bounds.  Counts are integers: every comparison of counts is exact equality.  J, precision and recall are one float64 division
of exact integers each, F a handful of float64 operations on them: compared within 1 ulp of float64."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mask_eval_rule as MR  # noqa: E402

from hamer_yolo_amd import lib as L  # noqa: E402
from hamer_yolo_amd.hamer.utils import mask_eval as ME  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")

# (H, W, r): one row / one column; a word that is not full; exactly one word; three words and three strips of rows; a short wide
# image; the largest radius (the disk reaches past the image and two words away); a radius above 32 on a tall image; and one
# image of many words and strips
SHAPES = [(1, 17, 2), (23, 1, 2), (37, 53, 0), (37, 53, 1), (37, 53, 3), (64, 64, 2), (70, 131, 5), (9, 200, 4), (70, 131, 64),
          (130, 67, 33), (150, 700, 7)]


def _single(H, W, y, x):
    s = np.zeros((H, W), bool)
    if 0 <= y < H and 0 <= x < W:
        s[y, x] = True
    return s


def image_pairs(H, W, r):
    """[(name, pred, gt)] of one shape."""
    a = MR.blobs(H, W, 11)
    empty, full = np.zeros((H, W), bool), np.ones((H, W), bool)
    border = np.zeros((H, W), bool)
    border[0, :] = border[-1, :] = border[:, 0] = border[:, -1] = True           # all four borders and the bottom-right pixel
    corner = _single(H, W, H - 1, W - 1)
    chk = (np.indices((H, W)).sum(0) % 2).astype(bool)
    pairs = [("blobs/shifted", a, np.roll(a, (1, 2), (0, 1))), ("blobs/other", a, MR.blobs(H, W, 12)), ("identical", a, a.copy()),
             ("empty pred", empty, a), ("empty gt", a, empty), ("both empty", empty, empty), ("full/blob", full, a),
             ("blob/full", a, full), ("border/blob", border, a), ("border/border", border, border.copy()),
             ("corner/blob", corner, a), ("blob/corner", a, corner), ("checkerboard/blob", chk, a), ("checkerboard/inverse", chk, ~chk)]
    # single pixels d apart along the longer axis: their 2 x 2 boundary blocks are then d - 1 .. d + 1 apart, so d = r + 2 is
    # further than r for every pair of boundary pixels, d = r + 1 and d = r have pairs exactly at r, d = r - 1 is inside
    for d in (r + 2, r + 1, r, r - 1):
        if d < 1:
            continue
        along_x = W >= H
        if 2 + d >= (W if along_x else H):
            continue
        y0, x0 = min(2, H - 1), min(2, W - 1)
        p = _single(H, W, y0, x0)
        g = _single(H, W, y0, x0 + d) if along_x else _single(H, W, y0 + d, x0)
        pairs.append((f"pixels {d} apart", p, g))
    if r == 5:                                                                   # offset (3, 4): exactly at the radius, off the axes
        pairs.append(("pixels (3, 4) apart", _single(H, W, 20, 20), _single(H, W, 23, 24)))
        pairs.append(("pixels (3, 5) apart", _single(H, W, 20, 20), _single(H, W, 23, 25)))
    return pairs


def to_device(pairs, label=3):
    """One frame per pair: pred_id 0 on pred pixels and -1 elsewhere, mask ``label`` on gt pixels."""
    pid = np.stack([np.where(p, 0, -1).astype(np.int32) for _, p, _ in pairs])
    m = np.stack([np.where(g, label, 0).astype(np.uint8) for _, _, g in pairs])
    return torch.from_numpy(pid).to(DEV), torch.from_numpy(m).to(DEV)


def within_one_ulp(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return bool(np.all(np.abs(got - want) <= np.spacing(np.abs(want))))


def abi(pid, mask, queries, r, counts=None, ws=None, fill=0xA5):
    """hm_mask_score itself: ``queries`` an (Q, 4) array uploaded as it is (no frame check), counts and the workspace
    pre-filled with ``fill`` bytes.  Returns (counts int64 (Q, 8) on the device, the workspace)."""
    lib = L.load()
    N, H, W = pid.shape
    q = np.ascontiguousarray(np.asarray(queries, np.int32).reshape(-1, 4))
    Q = len(q)
    qd = torch.from_numpy(q).to(DEV) if Q else None
    if counts is None:
        counts = torch.full((Q, 8 * 8), fill, dtype=torch.uint8, device=DEV).view(torch.int64)
    need = int(lib.hm_mask_score_workspace_bytes(Q, H, W, r))
    if ws is None:
        ws = torch.full((need,), fill, dtype=torch.uint8, device=DEV)
    L.check(lib.hm_mask_score(L.ptr(pid), L.ptr(mask), N, H, W, L.ptr(qd), Q, r, L.ptr(counts), L.ptr(ws), ws.numel(),
                              L.current_stream()), "hm_mask_score")
    return counts, ws


# ------------------------------------------------------------------ the kernel against the rule
@pytest.mark.parametrize("H,W,r", SHAPES)
def test_counts_equal_the_rule(H, W, r):
    pairs = image_pairs(H, W, r)
    pid, mask = to_device(pairs)
    queries = [(n, 0, 1, 3) for n in range(len(pairs))]
    got = ME.mask_counts(pid, mask, queries, radius=r)
    assert got.dtype == torch.int64 and tuple(got.shape) == (len(pairs), 8) and got.is_cuda
    got = got.cpu().numpy()
    want = np.stack([MR.counts(p, g, r) for _, p, g in pairs])
    for n, (name, _, _) in enumerate(pairs):
        assert np.array_equal(got[n], want[n]), (name, got[n].tolist(), want[n].tolist())
    raw, _ = abi(pid, mask, queries, r)                                          # 0xA5 in counts and workspace beforehand
    assert np.array_equal(raw.cpu().numpy(), want)
    s = ME.jf_from_counts(torch.from_numpy(got).to(DEV))
    ref = np.array([MR.jf(c) for c in want])
    for k, name in enumerate(("J", "F", "precision", "recall")):
        assert s[name].dtype == np.float64 and within_one_ulp(s[name], ref[:, k]), name
    by = {name: n for n, (name, _, _) in enumerate(pairs)}
    n = by["identical"]
    assert s["J"][n] == s["F"][n] == s["precision"][n] == s["recall"][n] == 1.0
    n = by["both empty"]
    assert got[n].tolist() == [0, 0, 0, 0, 0, 0, 0, H * W] and s["J"][n] == s["F"][n] == 1.0
    n = by["full/blob"]
    assert got[n, 3] == 0 and got[n, 1] == H * W and s["precision"][n] == 1.0          # a full frame has no boundary
    if f"pixels {r + 2} apart" in by:
        assert got[by[f"pixels {r + 2} apart"], 5:7].tolist() == [0, 0]
    if r >= 2 and f"pixels {r - 1} apart" in by:
        n = by[f"pixels {r - 1} apart"]
        assert (got[n, 5] > 0 and got[n, 6] > 0)
    if r == 5:
        assert got[by["pixels (3, 4) apart"], 5:7].tolist() == [4, 4] and got[by["pixels (3, 5) apart"], 5] < 4
    ME.release_workspaces()


def test_default_radius_is_bound_radius():
    H, W = 130, 260                                                               # ceil(0.008 * 290.7) = 3
    pairs = image_pairs(H, W, 3)[:3]
    pid, mask = to_device(pairs)
    queries = [(n, 0, 1, 3) for n in range(3)]
    assert ME.bound_radius(H, W) == 3
    want = np.stack([MR.counts(p, g, 3) for _, p, g in pairs])
    assert np.array_equal(ME.mask_counts(pid, mask, queries).cpu().numpy(), want)
    assert np.array_equal(ME.mask_counts(pid, mask, queries, bound_th=5).cpu().numpy(), np.stack([MR.counts(p, g, 5) for _, p, g in pairs]))
    out = torch.full((3, 8), -7, dtype=torch.int64, device=DEV)
    assert ME.mask_counts(pid, mask, queries, counts=out) is out and np.array_equal(out.cpu().numpy(), want)
    ME.release_workspaces()


# ------------------------------------------------------------------ batch and query handling
def _batch():
    """N = 3 frames of 37 x 53: frame 0 holds two meshes (ids 0 and 1) and two labels (3 and 5), frame 1 mesh 2 and label 7,
    frame 2 mesh 3 and label 3 -- and no query names frame 2."""
    H, W = 37, 53
    pid = np.full((3, H, W), -1, np.int32)
    mask = np.zeros((3, H, W), np.uint8)
    a, b = MR.blobs(H, W, 21), MR.blobs(H, W, 22)
    pid[0][a] = 0
    pid[0][b & ~a] = 1
    mask[0][np.roll(a, 2, 1)] = 3
    mask[0][np.roll(b, -2, 0) & ~np.roll(a, 2, 1)] = 5
    pid[1][MR.blobs(H, W, 23)] = 2
    mask[1][MR.blobs(H, W, 24)] = 7
    pid[2][MR.blobs(H, W, 25)] = 3
    mask[2][MR.blobs(H, W, 26)] = 3
    queries = [(0, 0, 1, 3), (0, 1, 2, 5), (0, 0, 2, -1), (1, 2, 3, 7), (1, 4, 4, 7), (1, 2, 3, -1), (3, 0, 5, 3)]
    order = np.random.default_rng(4).permutation(len(queries))
    return pid, mask, [queries[i] for i in order]


def test_batch_and_queries():
    pid_h, mask_h, queries = _batch()
    r = 3
    pid, mask = torch.from_numpy(pid_h).to(DEV), torch.from_numpy(mask_h).to(DEV)
    got = abi(pid, mask, queries, r)[0].cpu().numpy()
    want = MR.query_counts(pid_h, mask_h, queries, r)
    assert np.array_equal(got, want), (got.tolist(), want.tolist())
    k = queries.index((3, 0, 5, 3))
    assert got[k].tolist() == [0] * 8                                             # frame = N: zeros, pixels included
    k = queries.index((1, 4, 4, 7))
    assert got[k, 1] == 0 and got[k, 3] == 0 and got[k, 2] > 0 and got[k, 7] == 37 * 53      # an empty id range: an empty pred
    k = queries.index((0, 0, 2, -1))
    assert got[k, 1] == (pid_h[0] >= 0).sum() and got[k, 2] == (mask_h[0] != 0).sum()
    for i, q in enumerate(queries):                                               # each row equals the row it gets alone
        alone = abi(pid, mask, [q], r)[0].cpu().numpy()
        assert np.array_equal(alone[0], got[i]), q
    back = abi(pid, mask, queries[::-1], r)[0].cpu().numpy()
    assert np.array_equal(back[::-1], got)
    # the wrapper checks frames before the upload, and the other inputs
    with pytest.raises(ValueError, match="frame 3"):
        ME.mask_counts(pid, mask, queries, radius=r)
    ok = [q for q in queries if q[0] < 3]
    assert np.array_equal(ME.mask_counts(pid, mask, ok, radius=r).cpu().numpy(), MR.query_counts(pid_h, mask_h, ok, r))
    for bad in (dict(pred_id=pid.to(torch.int64)), dict(mask=mask.to(torch.int32)), dict(mask=mask[:2]), dict(pred_id=pid[0]),
                dict(mask=mask.cpu()), dict(radius=65), dict(radius=-1), dict(pred_id=pid.permute(0, 2, 1), mask=mask.permute(0, 2, 1)),
                dict(counts=torch.zeros(len(ok), 8, dtype=torch.int32, device=DEV))):
        kw = dict(pred_id=pid, mask=mask, radius=r)
        kw.update(bad)
        with pytest.raises(ValueError):
            ME.mask_counts(kw.pop("pred_id"), kw.pop("mask"), ok, **kw)
    ME.release_workspaces()


def test_buffers_and_determinism():
    pid_h, mask_h, queries = _batch()
    r = 3
    pid, mask = torch.from_numpy(pid_h).to(DEV), torch.from_numpy(mask_h).to(DEV)
    want = MR.query_counts(pid_h, mask_h, queries, r)
    a, ws = abi(pid, mask, queries, r)
    b, _ = abi(pid, mask, queries, r, fill=0x00)
    assert np.array_equal(a.cpu().numpy(), want) and torch.equal(a, b)
    again, _ = abi(pid, mask, queries, r, counts=a.clone(), ws=ws)                 # stale counts and a used workspace
    assert torch.equal(again, a)
    big = torch.full((ws.numel() * 3 + 64,), 0x5A, dtype=torch.uint8, device=DEV)
    c, _ = abi(pid, mask, queries, r, ws=big)
    assert torch.equal(c, a) and bool((big[ws.numel():] == 0x5A).all())            # nothing is written past what was asked for
    empty = ME.mask_counts(pid, mask, [], radius=r)
    assert tuple(empty.shape) == (0, 8) and empty.dtype == torch.int64 and empty.is_cuda
    assert tuple(abi(pid, mask, np.zeros((0, 4), np.int32), r)[0].shape) == (0, 8)
    ME.release_workspaces()


def test_mask_evaluator():
    pid_h, mask_h, queries = _batch()
    queries = [q for q in queries if q[0] < 3]
    pid, mask = torch.from_numpy(pid_h).to(DEV), torch.from_numpy(mask_h).to(DEV)
    ev = ME.MaskEvaluator()
    parts = (queries[:2], queries[2:3], queries[3:])
    for part in parts:
        out = ev(pid, mask, part, radius=3)
        assert torch.is_tensor(out) and out.is_cuda and tuple(out.shape) == (len(part), 8)
    want = MR.query_counts(pid_h, mask_h, queries, 3)
    assert ev.n == len(queries) and np.array_equal(ev.counts(), want)
    single = np.concatenate([ME.mask_counts(pid, mask, part, radius=3).cpu().numpy() for part in parts])
    assert np.array_equal(ev.counts(), single)
    ref = np.array([MR.jf(c) for c in want])
    per = ev.per_query()
    for k, name in enumerate(("J", "F", "precision", "recall")):
        assert within_one_ulp(per[name], ref[:, k])
    res = ev.result()
    assert sorted(res) == ["f_mean", "f_recall", "j_mean", "j_recall", "jf_mean", "n"] and res["n"] == len(queries)
    assert abs(res["j_mean"] - ref[:, 0].mean()) <= 1e-15 and abs(res["f_mean"] - ref[:, 1].mean()) <= 1e-15
    assert res["j_recall"] == (ref[:, 0] > 0.5).mean() and res["f_recall"] == (ref[:, 1] > 0.5).mean()
    assert abs(res["jf_mean"] - (ref[:, 0].mean() + ref[:, 1].mean()) / 2) <= 1e-15
    host = ME.MaskEvaluator()(pid, mask, queries[:2], sync=True, radius=3)
    assert isinstance(host, np.ndarray) and np.array_equal(host, want[:2])
    ME.release_workspaces()


# ------------------------------------------------------------------ end to end, synthetic MANO model
class _Cfg:
    ckpt_path = "synthetic:0"
    model_cfg = None
    use_onnx = False
    onnx_path = None


def _record(rng, hi, H, W, sides):
    """A record with a hand per side in ``sides``, placed so that it covers some tens of pixels of an H x W frame."""
    from hamer_yolo_amd import render
    f = render.default_camera(H, W, hi.cfg)[0, 0]
    z = f * 0.2 / (0.45 * min(H, W))
    rec = {"right": None, "left": None}
    for side in sides:
        dx = (-0.2 if side == "right" else 0.2) * W * z / f
        pg, ph = rng.normal(0, 0.3, 3).astype(np.float32), rng.normal(0, 0.15, 45).astype(np.float32)
        rec[side] = {"betas": rng.normal(0, 0.5, 10).astype(np.float32), "theta": np.concatenate([pg, ph]), "pose_hand": ph,
                     "pose_global": pg, "cam_t": np.array([dx, 0.0, z], np.float32), "is_right": side == "right"}
    return rec


def test_score_folder_end_to_end(tmp_path, capsys):
    from PIL import Image
    from hamer_yolo_amd import evaluate_masks as EM
    from hamer_yolo_amd import infer, render
    hi = infer.hamer_inference(_Cfg)
    img_dir, npy_dir, map_dir, roll_dir = (tmp_path / d for d in ("rgb", "npy", "maps", "rolled"))
    for d in (img_dir, npy_dir, roll_dir):
        d.mkdir()
    rng = np.random.default_rng(8)
    sizes = {"a0": (96, 128), "a1": (96, 128), "a2": (96, 128), "b0": (80, 112), "b1": (80, 112), "c0": (96, 128)}
    sides = {"a0": ("right", "left"), "a1": ("right",), "a2": ("left",), "b0": ("right", "left"), "b1": ("right",), "c0": ()}
    for stem, (H, W) in sizes.items():
        Image.fromarray(np.zeros((H, W, 3), np.uint8)).save(img_dir / f"{stem}.png")
        np.save(npy_dir / f"{stem}.npy", _record(rng, hi, H, W, sides[stem]))
    assert render.hand_maps_folder(str(img_dir), str(npy_dir), str(map_dir), hi, label=3, frames_per_pass=2) == 6
    maps = {s: np.load(map_dir / f"{s}.npy") for s in sizes}
    assert all((maps[s] == 3).any() and not (maps[s] == 3).all() for s in sizes if sides[s]) and not maps["c0"].any()

    # the maps against themselves: J = F = 1 on every frame, the hand-less one included
    res = EM.score_folder(str(img_dir), str(npy_dir), str(map_dir), hi, frames_per_pass=2)
    assert sorted(res["frames"]) == sorted(sizes) and res["n"] == 6 and res["n_skipped"] == 0 and res["skipped"] == []
    assert all(v == {"J": 1.0, "F": 1.0, "precision": 1.0, "recall": 1.0} for v in res["frames"].values())
    assert res["j_mean"] == res["f_mean"] == res["jf_mean"] == res["j_recall"] == res["f_recall"] == 1.0
    assert render._ws == {} and ME._ws == {}

    # rolled masks: the rule on the host from the saved maps
    for s in sizes:
        np.save(roll_dir / f"{s}.npy", np.roll(maps[s], (2, -3), (0, 1)))
    res = EM.score_folder(str(img_dir), str(npy_dir), str(roll_dir), hi, frames_per_pass=4)
    want = {}
    for s, (H, W) in sizes.items():
        want[s] = MR.jf(MR.counts(maps[s] == 3, np.roll(maps[s], (2, -3), (0, 1)) == 3, ME.bound_radius(H, W)))
    for s in sizes:
        got = res["frames"][s]
        assert within_one_ulp([got["J"], got["F"], got["precision"], got["recall"]], want[s]), s
    assert 0 < res["j_mean"] < 1 and abs(res["j_mean"] - np.mean([w[0] for w in want.values()])) <= 1e-15
    assert abs(res["f_mean"] - np.mean([w[1] for w in want.values()])) <= 1e-15
    wide = EM.score_folder(str(img_dir), str(npy_dir), str(roll_dir), hi, bound_th=6)
    for s, (H, W) in sizes.items():                                             # a radius in pixels: 6 covers the (2, -3) shift
        w6 = MR.jf(MR.counts(maps[s] == 3, np.roll(maps[s], (2, -3), (0, 1)) == 3, 6))
        got = wide["frames"][s]
        assert within_one_ulp([got["J"], got["F"], got["precision"], got["recall"]], w6) and got["F"] >= res["frames"][s]["F"], s

    # a missing mask, a mask of another size, a hand-less record against a mask with hand pixels
    os.remove(roll_dir / "a1.npy")
    np.save(roll_dir / "b0.npy", np.zeros((96, 128), np.uint8))
    blob = np.where(MR.blobs(96, 128, 31), 3, 0).astype(np.uint8)
    np.save(roll_dir / "c0.npy", blob)
    capsys.readouterr()
    res2 = EM.score_folder(str(img_dir), str(npy_dir), str(roll_dir), hi)
    printed = capsys.readouterr().out
    assert sorted(res2["skipped"]) == ["a1", "b0"] and res2["n_skipped"] == 2 and res2["n"] == 4
    assert "Skipping a1" in printed and "Skipping b0" in printed
    assert sorted(res2["frames"]) == ["a0", "a2", "b1", "c0"]
    assert res2["frames"]["c0"] == {"J": 0.0, "F": 0.0, "precision": 1.0, "recall": 0.0}
    assert res2["frames"]["a0"] == res["frames"]["a0"] and res2["frames"]["b1"] == res["frames"]["b1"]
    other = EM.score_folder(str(img_dir), str(npy_dir), str(roll_dir), hi, label=4)          # no pixel carries label 4
    assert all(v["J"] == 0.0 for s, v in other["frames"].items() if sides[s]) and other["frames"]["c0"]["J"] == 1.0

    # rank / world partition the records
    halves = [EM.score_folder(str(img_dir), str(npy_dir), str(map_dir), hi, rank=k, world=2) for k in (0, 1)]
    assert not set(halves[0]["frames"]) & set(halves[1]["frames"])
    assert sorted(set(halves[0]["frames"]) | set(halves[1]["frames"])) == sorted(sizes) and halves[0]["n"] + halves[1]["n"] == 6

    # the driver
    import json
    from unittest import mock
    out_json = tmp_path / "r.json"
    with mock.patch.object(infer, "hamer_inference", lambda cfg: hi):
        capsys.readouterr()
        got = EM.main(["--pred", str(npy_dir), "--images", str(img_dir), "--masks", str(map_dir), "--json", str(out_json)])
        line = capsys.readouterr().out.splitlines()[-1]
    assert got["n"] == 6 and "6 frames: J mean 1.0000" in line and "skipped 0" in line
    saved = json.loads(out_json.read_text())
    assert saved["frames"] == got["frames"] and saved["n"] == 6 and saved["label"] == 3 and saved["bound_th"] == 0.008
    with pytest.raises(ValueError):
        EM.score_folder(str(img_dir), str(npy_dir), str(map_dir), hi, label=0)
