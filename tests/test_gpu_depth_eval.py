"""GPU: hm_depth_residuals against the numpy rule of tests/depth_eval_rule.py where vectors, the per-workgroup query slots, the
bin window and contention can go wrong; its batch invariance and buffers; refine_cam_t against the numpy loop run on the GPU's
own renders; evaluate_depth's folder drivers and ``infer --depth-maps`` on a synthetic MANO model.

Bounds.  hist and counts are integers and the median is the centre of a bin: every comparison of them is exact equality
(NaN where the rule says NaN).  The mean, mean absolute value and rms are sums of at most 4096 fp64 products in a fixed order
followed by one division (and a square root): compared to 1e-12 relative, the bound the rule's own statement leaves to the
square root and to nothing else.  The refined depth is within 2 mm (four bins) of the truth."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import depth_eval_rule as DR  # noqa: E402

from hamer_yolo_amd import lib as L  # noqa: E402
from hamer_yolo_amd import render  # noqa: E402
from hamer_yolo_amd.hamer.utils import depth_eval as DE  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def check(got, depth, pid, sensor, mq, Q, **kw):
    """``got`` (a depth_residuals dict) equals the rule on the host arrays."""
    rule = {k: v for k, v in kw.items() if k in ("unit", "bin_m", "bins", "raw_range", "mask", "labels")}
    hist, counts = DR.residuals(depth, pid, sensor, mq, Q, **rule)
    st = DR.stats(hist, counts, rule.get("bin_m", 0.0005))
    gh, gc, gs = got["hist"].cpu().numpy(), got["counts"].cpu().numpy(), got["stats"].cpu().numpy()
    assert gh.dtype == np.int32 and gc.dtype == np.int64 and gs.dtype == np.float64
    assert gh.shape == hist.shape and gc.shape == (Q, 8) and gs.shape == (Q, 4)
    assert np.array_equal(gc, counts), (gc.tolist(), counts.tolist())
    assert np.array_equal(gh, hist), np.argwhere(gh != hist)[:8].tolist()
    assert np.array_equal(gs[:, 0], st[:, 0], equal_nan=True), (gs[:, 0].tolist(), st[:, 0].tolist())
    assert np.array_equal(np.isnan(gs), np.isnan(st))
    ok = ~np.isnan(st)
    assert (np.abs(gs[ok] - st[ok]) <= 1e-12 * np.abs(st[ok])).all(), (gs.tolist(), st.tolist())
    return hist, counts, st


def run(depth, pid, sensor, mq, Q, **kw):
    args = dict(kw)
    mask, labels = args.pop("mask", None), args.pop("labels", None)
    got = DE.depth_residuals(dev(depth), dev(pid), dev(sensor), mq, Q, mask=dev(mask), labels=labels, **args)
    return got, check(got, depth, pid, sensor, mq, Q, **kw)


def random_maps(seed, N, H, W, ids, spread, base=(0.3, 0.9), cover=0.6):
    rng = np.random.default_rng(seed)
    pid = rng.choice(np.asarray(ids, np.int32), (N, H, W))
    pid[rng.random((N, H, W)) > cover] = -1
    depth = np.where(pid >= 0, rng.uniform(*base, (N, H, W)), 0.0).astype(np.float32)
    sensor = np.rint((depth + rng.normal(0, spread, (N, H, W))) * 1000.0).clip(0, 65535).astype(np.uint16)
    sensor[rng.random((N, H, W)) < 0.1] = 0
    mask = rng.choice(np.array([0, 3, 5], np.uint8), (N, H, W))
    return depth, pid, sensor, mask


def abi(depth, pid, sensor, mq, Q, unit=0.001, raw=(1, 65535), bin_m=0.0005, bins=4096, mask=None, labels=None, fill=0xA5):
    """hm_depth_residuals itself, the outputs and the workspace pre-filled with ``fill`` bytes."""
    lib = L.load()
    N, H, W = pid.shape
    out = {"hist": torch.full((Q, bins * 4), fill, dtype=torch.uint8, device=DEV).view(torch.int32),
           "counts": torch.full((Q, 64), fill, dtype=torch.uint8, device=DEV).view(torch.int64),
           "stats": torch.full((Q, 32), fill, dtype=torch.uint8, device=DEV).view(torch.float64)}
    need = int(lib.hm_depth_residuals_workspace_bytes(Q, bins))
    ws = torch.full((need + 64,), fill, dtype=torch.uint8, device=DEV)
    mqd = dev(np.asarray(mq, np.int32))
    L.check(lib.hm_depth_residuals(L.ptr(depth), L.ptr(pid), L.ptr(sensor), L.ptr(mask), L.ptr(labels), N, H, W, L.ptr(mqd), len(mq), Q,
                                   unit, raw[0], raw[1], bin_m, bins, L.ptr(out["hist"]) if Q else None, L.ptr(out["counts"]) if Q else None,
                                   L.ptr(out["stats"]) if Q else None, L.ptr(ws), need, L.current_stream()), "hm_depth_residuals")
    torch.cuda.synchronize()
    assert bool((ws[need:] == fill).all())                                            # nothing is written past what was asked for
    return out


# ------------------------------------------------------------------ 7: random maps, nothing a multiple of a vector
def test_random_maps():
    N, H, W = 3, 37, 53
    mq = [0, 1, 0, -1, 2]                                                             # meshes 0 and 2 share a query, mesh 3 counts for none
    for seed, spread in ((1, 0.004), (2, 0.05), (3, 0.4)):
        depth, pid, sensor, _ = random_maps(seed, N, H, W, [-3, -1, 0, 1, 2, 3, 4, 5, 7], spread)
        got, (hist, counts, st) = run(depth, pid, sensor, mq, 3)
        assert counts[:, 0].sum() == np.isin(pid, [0, 1, 2, 4]).sum() and (counts[:, 5] > 0).all()
        raw = abi(dev(depth), dev(pid), dev(sensor), mq, 3)                           # 0xA5 in every output beforehand
        assert all(torch.equal(raw[k], got[k]) or k == "stats" for k in raw)
        assert np.array_equal(raw["stats"].cpu().numpy(), got["stats"].cpu().numpy(), equal_nan=True)
    # residuals on bin edges up to the rounding of raw * 0.001: a fused multiply-subtract moves hundreds of these pixels to
    # the neighbouring bin (tests/test_depth_eval_host.py test_contraction_would_show)
    depth, pid, sensor = DR.contraction_maps(4, N, H, W, 5)
    run(depth, pid, sensor, mq, 3)
    # views that start at an address that is not 16-byte aligned: the scalar head and tail
    big = [dev(a) for a in random_maps(5, 1, 1, N * H * W + 3, [0, 1, 2, 4], 0.05)[:3]]
    for off in (1, 2, 3):
        d, i, s = (t.reshape(-1)[off:off + N * H * W].view(N, H, W) for t in big)
        assert i.data_ptr() % 16 == 4 * off and i.is_contiguous()
        got = DE.depth_residuals(d, i, s, mq, 3)
        check(got, d.cpu().numpy(), i.cpu().numpy(), s.cpu().numpy(), mq, 3)
    DE.release_workspaces()


# ------------------------------------------------------------------ 7b: more than one workgroup of the scan
def big_maps():
    """3 x 120 x 160 pixels -- a workgroup of the scan takes 32768 -- with eleven meshes on a smooth depth field: seven in the
    first workgroup's pixels, the disc of mesh 7 lying across pixel 32768 (row 84 of frame 1); the sensor is up to 4 mm off."""
    N, H, W = 3, 120, 160
    n, v, u = np.meshgrid(np.arange(N), np.arange(H), np.arange(W), indexing="ij")
    z = 0.5 + 2e-5 * u + 2e-5 * v + 0.003 * np.sin(u / 7.0) * np.cos(v / 5.0) + 0.01 * n
    sensor = np.rint((z + 0.004 * np.sin(u / 11.0 + v / 13.0 + n)) * 1000.0).astype(np.uint16)
    pid = np.full((N, H, W), -1, np.int32)
    for k in range(6):
        pid[0, 5 + 38 * (k // 3):40 + 38 * (k // 3), 4 + 52 * (k % 3):50 + 52 * (k % 3)] = k
    for frame, cv, cu, r, i in ((0, 100, 80, 18, 6), (1, 85, 80, 30, 7)):
        pid[frame][(v[0] - cv) ** 2 + (u[0] - cu) ** 2 <= r * r] = i
    pid[1, 2:30, 2:158], pid[2, 10:110, 10:150] = 8, 9
    pid[2][(v[0] - 60) ** 2 + (u[0] - 80) ** 2 <= 20 * 20] = 10
    pid[0, 0, :3], pid[2, -1, -3:] = 0, 9                                              # the scalar head and tail of an unaligned base are covered
    return np.where(pid >= 0, z, 0.0).astype(np.float32), pid, sensor


def test_more_than_one_workgroup():
    """Vector indices past the first workgroup's, and the scalar head and tail read by workgroup 0 alone."""
    depth, pid, sensor = big_maps()
    total, mq = pid.size, list(range(11))
    # by the rule alone: every query has pixels in range, and mesh 7 has some on both sides of pixel 32768
    at = np.arange(total).reshape(pid.shape)
    sides = [DR.residuals(depth, np.where(keep, pid, -1), sensor, mq, 11)[1] for keep in (at < 32768, at >= 32768)]
    assert total > 32768 and sides[0][7, 5] > 0 and sides[1][7, 5] > 0 and ((sides[0] + sides[1])[:, 5] > 0).all()
    got, (hist, counts, _) = run(depth, pid, sensor, mq, 11)
    assert np.array_equal(counts, sides[0] + sides[1]) and len(np.unique(pid[0][pid[0] >= 0])) == 7
    one, (hist1, counts1, _) = run(depth, pid, sensor, [0] * 11, 1)
    assert torch.equal(one["hist"][0], got["hist"].sum(0, dtype=torch.int32)) and torch.equal(one["counts"][0], got["counts"].sum(0))
    assert np.array_equal(hist1[0], hist.sum(0))
    # the same from a base 4 bytes past a 16-byte boundary: three pixels of head, one of tail (total % 4 == 0)
    flat = [torch.zeros(total + 8, dtype=t.dtype, device=DEV) for t in (dev(depth), dev(pid), dev(sensor))]   # mesh 0 around the view
    for t, a in zip(flat, (depth, pid, sensor)):
        t[1:1 + total] = dev(a).reshape(-1)
    d, i, s = (t[1:1 + total].view(pid.shape) for t in flat)
    assert i.data_ptr() % 16 == 4 and i.is_contiguous() and total % 4 == 0 and (pid.reshape(-1)[[0, 1, 2, -1]] >= 0).all()
    for q, Q in ((mq, 11), ([0] * 11, 1)):
        off = DE.depth_residuals(d, i, s, q, Q)
        check(off, depth, pid, sensor, q, Q)
        assert all(torch.equal(off[k], (got if Q == 11 else one)[k]) for k in ("hist", "counts"))
    DE.release_workspaces()


# ------------------------------------------------------------------ 8: residuals exactly on bin edges, both ends of the range
@pytest.mark.parametrize("bins", [2, 4096])
def test_bin_edges(bins):
    unit, bin_m = 2.0 ** -10, 2.0 ** -11
    rng = np.random.default_rng(bins)
    N, H, W = 2, 37, 53
    raw = rng.integers(1100, 3000, (N, H, W))
    off = rng.integers(-(bins // 2) - 2, bins // 2 + 3, (N, H, W))                    # floor(r / bin_m) itself: every edge, and two past both ends
    pid = rng.integers(0, 2, (N, H, W)).astype(np.int32)
    half = bins // 2
    ends = [-half - 2, -half - 1, -half, -half + 1, half - 2, half - 1, half, half + 1]   # both ends of the range, for both queries
    off.reshape(-1)[:16], pid.reshape(-1)[:16] = ends + ends, [0] * 8 + [1] * 8
    depth = ((2 * raw - off) * 2.0 ** -11).astype(np.float32)                         # exact in fp32: r = off * bin_m exactly
    assert np.array_equal(depth.astype(np.float64), (2 * raw - off) * 2.0 ** -11)
    _, (hist, counts, _) = run(depth, pid, raw.astype(np.uint16), [0, 1], 2, unit=unit, bin_m=bin_m, bins=bins)
    for q in range(2):
        k = off[pid == q] + bins // 2
        assert counts[q, 3] == (k < 0).sum() > 0 and counts[q, 4] == (k >= bins).sum() > 0
        assert np.array_equal(hist[q], np.bincount(k[(k >= 0) & (k < bins)], minlength=bins))
        assert hist[q, 0] > 0 and hist[q, bins - 1] > 0
    DE.release_workspaces()


# ------------------------------------------------------------------ 9: more queries in one workgroup than it keeps slots for
def test_nine_meshes_in_one_frame():
    depth, pid, sensor, _ = random_maps(9, 1, 64, 64, list(range(9)), 0.01, cover=1.0)
    _, (hist, counts, _) = run(depth, pid, sensor, list(range(9)), 9)
    assert (counts[:, 0] > 300).all() and counts[:, 0].sum() == 64 * 64
    # several meshes per query, in another order, and two frames: the same integers per query
    run(depth, pid, sensor, [2, 2, 1, 1, 0, 0, 2, 1, 0], 3)
    two = [np.concatenate([a, a[:, ::-1]]) for a in (depth, pid, sensor)]
    _, (hist2, counts2, _) = run(*two, list(range(9)), 9)
    assert np.array_equal(hist2, 2 * hist) and np.array_equal(counts2, 2 * counts)
    # a wide spread: most pixels fall outside their slot's window of bins
    depth, pid, sensor, _ = random_maps(10, 1, 64, 64, list(range(9)), 0.3, cover=1.0)
    run(depth, pid, sensor, list(range(9)), 9)
    DE.release_workspaces()


# ------------------------------------------------------------------ 10: every covered pixel in one bin
def test_maximum_contention():
    H = W = 64
    pid = np.zeros((1, H, W), np.int32)
    depth = np.full((1, H, W), 0.5, np.float32)
    sensor = np.full((1, H, W), 507, np.uint16)
    _, (hist, counts, st) = run(depth, pid, sensor, [0], 1)
    k = int(np.floor((507 * 0.001 - 0.5) / 0.0005)) + 2048
    assert hist[0, k] == H * W and hist[0].sum() == H * W and counts[0].tolist() == [H * W, 0, 0, 0, 0, H * W, 0, 0]
    assert st[0, 0] == st[0, 1] == st[0, 2] == (k - 2048 + 0.5) * 0.0005
    # the same in sixteen frames (several workgroups adding to one address), and everything below / above a two-bin histogram
    many = [np.repeat(a, 16, 0) for a in (depth, pid, sensor)]
    _, (hist, _, _) = run(*many, [0], 1)
    assert hist[0, k] == 16 * H * W
    _, (_, counts, st) = run(depth, pid, sensor, [0], 1, bins=2)
    assert counts[0].tolist() == [H * W, 0, 0, 0, H * W, 0, 0, 0] and np.isnan(st[0]).all()
    _, (_, counts, st) = run(depth + np.float32(0.1), pid, sensor, [0], 1, bins=2)
    assert counts[0].tolist() == [H * W, 0, 0, H * W, 0, 0, 0, 0] and np.isnan(st[0]).all()
    DE.release_workspaces()


# ------------------------------------------------------------------ 11: masks, the raw gate, no queries, empty queries
def test_masks_gate_and_empty_queries():
    N, H, W = 2, 37, 53
    depth, pid, sensor, mask = random_maps(11, N, H, W, [0, 1, 2, 3], 0.01)
    mq = [0, 1, 2, 3]
    plain, _ = run(depth, pid, sensor, mq, 5)                                          # query 4 has no mesh
    c = plain["counts"].cpu().numpy()
    assert c[4].tolist() == [0] * 8 and np.isnan(plain["stats"][4].cpu().numpy()).all() and int(plain["hist"][4].sum()) == 0
    for labels in ([-2] * 5, [-1] * 5, [3] * 5, [-2, -1, 3, 5, 0], [7] * 5):
        got, (_, counts, _) = run(depth, pid, sensor, mq, 5, mask=mask, labels=labels)
        if labels == [-2] * 5:
            assert all(torch.equal(got[k], plain[k]) for k in ("hist", "counts"))
        if labels == [7] * 5:
            assert np.array_equal(counts[:, 1], counts[:, 0]) and counts[:, 2:].sum() == 0
    # the ABI: a mask without labels and labels without a mask are no mask test
    d, i, s, m = dev(depth), dev(pid), dev(sensor), dev(mask)
    lab = dev(np.array([3] * 5, np.int32))
    for kw in (dict(mask=m), dict(labels=lab)):
        raw = abi(d, i, s, mq, 5, **kw)
        assert torch.equal(raw["hist"], plain["hist"]) and torch.equal(raw["counts"], plain["counts"])
    got, (_, counts, _) = run(depth, pid, sensor, mq, 5, raw_range=(450, 700))
    assert (counts[:4, 2] > c[:4, 2]).all()
    run(depth, pid, sensor, mq, 5, raw_range=(700, 700))
    run(depth, pid, sensor, [-1, -1, 9, -5], 5)                                        # no mesh counts for a query
    run(depth, pid, sensor, [], 2)                                                     # an empty mesh table
    empty = DE.depth_residuals(d, i, s, mq, 0)
    assert tuple(empty["hist"].shape) == (0, 4096) and tuple(empty["counts"].shape) == (0, 8) and tuple(empty["stats"].shape) == (0, 4)
    abi(d, i, s, mq, 0)
    for bad in (dict(bins=3), dict(bins=4098), dict(unit=0.0), dict(bin_m=float("nan")), dict(raw_range=(5, 4)), dict(mask=m),
                dict(labels=[3] * 5), dict(mask=m, labels=[3] * 4), dict(mask=m, labels=[256] * 5), dict(mask=m[:1], labels=[3] * 5)):
        with pytest.raises(ValueError):
            DE.depth_residuals(d, i, s, mq, 5, **bad)
    for bad in ((d.double(), i, s), (d, i.long(), s), (d, i, torch.zeros_like(i)), (d[:1], i, s), (d, i, s.cpu()), (d[0], i[0], s[0])):
        with pytest.raises(ValueError):
            DE.depth_residuals(*bad, mq, 5)
    DE.release_workspaces()


# ------------------------------------------------------------------ 12: a frame alone and inside a batch
def test_batch_independence():
    H, W = 37, 53
    frames = [random_maps(20 + n, 1, H, W, [0, 1], 0.02) for n in range(4)]
    alone = DE.depth_residuals(*[dev(a) for a in frames[2][:3]], [0, 1], 2)
    # in the batch frame n holds meshes 2 n and 2 n + 1, one query each
    batch = [np.concatenate([f[k] for f in frames]) for k in range(3)]
    batch[1] = np.concatenate([np.where(f[1] >= 0, f[1] + 2 * n, -1) for n, f in enumerate(frames)]).astype(np.int32)
    got = DE.depth_residuals(*[dev(a) for a in batch], list(range(8)), 8)
    check(got, *batch, list(range(8)), 8)
    for k in ("hist", "counts", "stats"):
        a, b = alone[k].cpu().numpy(), got[k][4:6].cpu().numpy()
        assert a.tobytes() == b.tobytes(), k
    ev = DE.DepthEvaluator()
    r = ev(*[dev(a) for a in frames[2][:3]], [0, 1], 2)
    assert r["hist"].is_cuda and ev.n == 2
    host = ev(*[dev(a) for a in batch], list(range(8)), 8, sync=True)
    assert isinstance(host["counts"], np.ndarray) and ev.n == 10
    assert np.array_equal(ev.counts()[:2], ev.counts()[6:8]) and np.array_equal(ev.hist()[:2], ev.hist()[6:8])
    per, want = ev.per_query(), DR.summary(ev.hist(), ev.counts(), 0.0005)
    for k in want:
        assert np.array_equal(per[k], want[k], equal_nan=True), k
    res = ev.result()
    assert res["hands"] == 10 and res["scored"] == np.isfinite(want["median"]).sum() and 0 < res["measured"] < 1
    DE.release_workspaces()


# ------------------------------------------------------------------ 13: refine_cam_t on the ellipsoid
SCENE = dict(H=240, W=320, K=np.array([[600.0, 0, 160.0], [0, 600.0, 120.0], [0, 0, 1.0]]), centre=np.array([0.03, -0.02, 0.5]),
             factors=(1.16, 0.85, 1.4, 1.16), wall=1.5, unit=0.001)


def test_refine_cam_t_on_the_ellipsoid():
    v, f = DR.ellipsoid()
    H, W, K, unit = SCENE["H"], SCENE["W"], SCENE["K"], SCENE["unit"]
    B = len(SCENE["factors"])
    faces = torch.from_numpy(f).to(DEV)

    def gpu_render(placed):
        meshes = [{"frame": j, "vertices": torch.from_numpy(placed[j]).to(DEV), "faces": faces} for j in range(len(placed))]
        r = render.render_views(H, W, K, meshes, outputs=("depth", "mesh_id"), views=B, device=DEV)
        return r["depth"].cpu().numpy(), r["mesh_id"].cpu().numpy()

    verts = np.repeat(v[None].astype(np.float32), B, 0)
    truth = (SCENE["centre"][None, :] * np.asarray(SCENE["factors"])[:, None]).astype(np.float32)
    depth, mid = gpu_render(verts + truth[:, None, :])
    assert all((mid[j] == j).sum() > 2000 for j in range(B))
    sensor = DR.sensor_from_depth(depth, unit, SCENE["wall"])
    sensor[3] = 0                                                                      # the fourth hand's frame measured nothing
    start = np.repeat(SCENE["centre"][None].astype(np.float32), B, 0)
    want = DR.refine(gpu_render, verts, start, sensor, unit)
    args = (H, W, K, dev(verts), faces, dev(start), list(range(B)), dev(sensor))
    got = DE.refine_cam_t(*args, unit=unit)
    cam_t = got["cam_t"].cpu().numpy()
    assert cam_t.dtype == np.float32 and cam_t.tobytes() == want[0].tobytes(), (cam_t.tolist(), want[0].tolist())
    assert np.array_equal(got["median"].cpu().numpy(), want[1], equal_nan=True) and np.array_equal(got["valid"].cpu().numpy(), want[2])
    assert got["updated"].cpu().numpy().tolist() == want[3].tolist() == [True, True, True, False]
    one = DE.refine_cam_t(*args, unit=unit, iterations=1)["cam_t"].cpu().numpy()
    assert one.tobytes() == want[4][0].tobytes()
    e0, e1, e2 = (np.abs(c[:3, 2].astype(np.float64) - truth[:3, 2]) for c in (start, one, cam_t))
    print("tz errors in mm: start", e0 * 1e3, "one step", e1 * 1e3, "two steps", e2 * 1e3)
    assert (e1 < e0).all() and (e2 <= 0.002).all()
    assert cam_t[3].tobytes() == start[3].tobytes() and np.isnan(want[1][3]) and want[2][3] == 0
    few = DE.refine_cam_t(*args, unit=unit, min_pixels=10 ** 6)                        # too few valid pixels: every hand keeps its bytes
    assert few["cam_t"].cpu().numpy().tobytes() == start.tobytes() and not bool(few["updated"].any())
    assert np.isfinite(few["median"][:3].cpu().numpy()).all()
    render.release_workspaces()
    DE.release_workspaces()


# ------------------------------------------------------------------ 14: the drivers, synthetic MANO model
class _Cfg:
    ckpt_path = "synthetic:0"
    model_cfg = None
    use_onnx = False
    onnx_path = None


FH, FW = 192, 256
FK = np.array([[300.0, 0.0, 128.0], [0.0, 300.0, 96.0], [0.0, 0.0, 1.0]])
FACTOR = {"right": 1.1, "left": 0.92}                                                 # truth = prediction scaled along its ray


def _true_record(rng, sides):
    rec = {"right": None, "left": None}
    for side in sides:
        pg, ph = rng.normal(0, 0.3, 3).astype(np.float32), rng.normal(0, 0.15, 45).astype(np.float32)
        rec[side] = {"betas": rng.normal(0, 0.5, 10).astype(np.float32), "theta": np.concatenate([pg, ph]), "pose_hand": ph,
                     "pose_global": pg, "cam_t": np.array([-0.12 if side == "right" else 0.12, 0.0, 0.7], np.float32),
                     "is_right": side == "right"}
    return rec


def _same(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    if isinstance(a, float) and np.isnan(a):
        return isinstance(b, float) and np.isnan(b)
    return type(a) is type(b) and a == b


def test_folder_drivers(tmp_path, capsys):
    from PIL import Image
    from hamer_yolo_amd import evaluate_depth as ED
    from hamer_yolo_amd import infer
    hi = infer.hamer_inference(_Cfg)
    npy_dir, depth_dir, out_dir = tmp_path / "npy", tmp_path / "depth", tmp_path / "refined"
    npy_dir.mkdir(); depth_dir.mkdir()
    rng = np.random.default_rng(14)
    sides = {"a0": ("right", "left"), "a1": ("right",), "a2": ("left",), "a3": ("right",)}
    truth = {s: _true_record(rng, sides[s]) for s in sides}
    faces = torch.as_tensor(np.asarray(hi.mano.faces, np.int32), device=DEV)
    for n, (stem, rec) in enumerate(truth.items()):
        hands = [rec[t] for t in sides[stem]]
        verts = render.camera_vertices(hi, hands)
        meshes = [{"frame": 0, "vertices": verts[j], "faces": faces} for j in range(len(hands))]
        depth = render.render_views(FH, FW, FK, meshes, outputs=("depth",), views=1, device=DEV)["depth"][0].cpu().numpy()
        raw = DR.sensor_from_depth(depth, 0.001, 1.5)
        if stem == "a3":
            pass                                                                       # a3 is given no depth map
        elif n % 2:
            np.save(depth_dir / f"{stem}.npy", raw)
        else:
            Image.fromarray(raw).save(depth_dir / f"{stem}.png")
        pred = {t: (None if rec[t] is None else dict(rec[t], cam_t=(rec[t]["cam_t"].astype(np.float64) / FACTOR[t]).astype(np.float32)))
                for t in ("right", "left")}
        np.save(npy_dir / f"{stem}.npy", pred)

    capsys.readouterr()
    res = ED.score_folder(str(npy_dir), str(depth_dir), hi, FK, frames_per_pass=2)
    assert "Skipping a3" in capsys.readouterr().out and res["skipped"] == ["a3"] and res["n_skipped"] == 1
    assert [(r["stem"], r["hand"]) for r in res["rows"]] == [("a0", "right"), ("a0", "left"), ("a1", "right"), ("a2", "left")]
    assert res["hands"] == res["scored"] == 4 and render._ws == {} and DE._ws == {}
    for r in res["rows"]:
        tz = 0.7 / FACTOR[r["hand"]]
        print(r["stem"], r["hand"], "median residual %.4f m, expected about %.4f" % (r["median_m"], 0.7 - tz), r["counts"])
        assert np.sign(r["median_m"]) == np.sign(FACTOR[r["hand"]] - 1) and abs(r["median_m"] - (0.7 - tz)) < 0.02
        assert r["counts"][0] >= 200 and 0 < r["measured"] <= 1
    assert res["median_abs_mm"] > 40 and set(res["inliers"]) == {"5mm", "10mm", "20mm"}
    # the same counts from DepthEvaluator called by hand, one frame at a time
    ev = DE.DepthEvaluator()
    for stem in ("a0", "a1", "a2"):
        rec = np.load(npy_dir / f"{stem}.npy", allow_pickle=True).item()
        hands = [rec[t] for t in sides[stem]]
        verts = render.camera_vertices(hi, hands)
        meshes = [{"frame": 0, "vertices": verts[j], "faces": faces} for j in range(len(hands))]
        r = render.render_views(FH, FW, FK, meshes, outputs=("depth", "mesh_id"), views=1, device=DEV)
        sensor = ED.load_depth(ED.find_depth(str(depth_dir), stem), (FH, FW), 0.001)
        ev(r["depth"], r["mesh_id"], dev(sensor[None]), list(range(len(hands))), len(hands))
    assert [r["counts"] for r in res["rows"]] == ev.counts()[:, :6].tolist()
    assert res["median_abs_mm"] == ev.result()["median_abs_mm"]
    halves = [ED.score_folder(str(npy_dir), str(depth_dir), hi, FK, rank=k, world=2) for k in (0, 1)]
    assert sorted(r["stem"] + r["hand"] for h in halves for r in h["rows"]) == sorted(r["stem"] + r["hand"] for r in res["rows"])

    # refine: within 2 mm of the truth; a hand given no depth keeps every existing key
    st = ED.refine_folder(str(npy_dir), str(depth_dir), str(out_dir), hi, FK, frames_per_pass=2)
    assert st == {"records": 4, "hands": 5, "refined": 4, "skipped": ["a3"], "n_skipped": 1}
    for stem in sides:
        before = np.load(npy_dir / f"{stem}.npy", allow_pickle=True).item()
        after = np.load(out_dir / f"{stem}.npy", allow_pickle=True).item()
        for t in ("right", "left"):
            if before[t] is None:
                assert after[t] is None
                continue
            a, b = after[t], before[t]
            assert set(a) == set(b) | set(ED.NEW_KEYS) and all(_same(a[k], b[k]) for k in b if k != "cam_t")
            assert _same(a["cam_t_unrefined"], b["cam_t"]) and a["cam_t"].dtype == np.float32 and a["cam_t"].shape == (3,)
            if stem == "a3":
                assert _same(a["cam_t"], b["cam_t"]) and a["depth_refined"] is False and a["depth_pixels"] == 0 and np.isnan(a["depth_residual_m"])
            else:
                err = abs(float(a["cam_t"][2]) - 0.7)
                print(stem, t, "tz %.5f, %.2f mm from the truth; last median %.4f m over %d pixels" %
                      (a["cam_t"][2], err * 1e3, a["depth_residual_m"], a["depth_pixels"]))
                assert a["depth_refined"] is True and a["depth_pixels"] >= 200 and err <= 0.002
                assert np.allclose(a["cam_t"][:2] / a["cam_t"][2], b["cam_t"][:2] / b["cam_t"][2], rtol=1e-5)
    again = ED.score_folder(str(out_dir), str(depth_dir), hi, FK)
    assert again["median_abs_mm"] <= 2.0 and again["inliers"]["5mm"] > res["inliers"]["5mm"]


def test_infer_depth_maps_in_a_child_process(tmp_path):
    """``infer --masks ... --depth-maps DIR`` is the folder job followed by refine_folder(output, DIR, output): undoing the
    child's refinement and refining here gives the child's records."""
    from PIL import Image
    from hamer_yolo_amd import evaluate_depth as ED
    from hamer_yolo_amd import infer, synth
    H, W = 240, 320
    rgb, masks, depth, out = (tmp_path / d for d in ("rgb", "masks", "depth", "out"))
    for d in (rgb, masks, depth):
        d.mkdir()
    K = np.array([[400.0, 0, 160.0], [0, 400.0, 120.0], [0, 0, 1.0]], np.float32)
    np.savetxt(tmp_path / "K.txt", K)
    for i in range(2):
        Image.fromarray(synth.frame_u8(H, W, seed=70 + i).numpy()[:, :, ::-1]).save(rgb / f"g{i}.png")
        m = np.zeros((H, W), np.uint8)
        m[60 + 20 * i:160 + 20 * i, 90:200] = 3
        np.save(masks / f"g{i}.npy", m)
        np.save(depth / f"g{i}.npy", np.full((H, W), 3000 + 50 * i, np.uint16))     # a wall near where the synthetic model puts its hands
    cmd = [sys.executable, "-m", "hamer_yolo_amd.infer", "--input", str(rgb), "--output", str(out), "--masks", str(masks),
           "--intrinsics", str(tmp_path / "K.txt"), "--ckpt", "synthetic:0", "--depth-maps", str(depth)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "hands moved onto" in r.stdout
    child = {s: np.load(out / f"{s}.npy", allow_pickle=True).item() for s in ("g0", "g1")}
    undone, here = tmp_path / "undone", tmp_path / "here"
    undone.mkdir()
    for s, rec in child.items():
        assert rec["right"] is not None and set(ED.NEW_KEYS) <= set(rec["right"])
        plain = {t: (None if rec[t] is None else {k: (rec[t]["cam_t_unrefined"] if k == "cam_t" else v) for k, v in rec[t].items()
                                                   if k not in ED.NEW_KEYS}) for t in ("right", "left")}
        np.save(undone / f"{s}.npy", plain)
    hi = infer.hamer_inference(_Cfg)
    ED.refine_folder(str(undone), str(depth), str(here), hi, infer.load_intrinsics(str(tmp_path / "K.txt")), image_folder=str(rgb))
    for s in child:
        mine = np.load(here / f"{s}.npy", allow_pickle=True).item()
        print(s, {k: mine["right"][k] for k in ("cam_t", "cam_t_unrefined", "depth_residual_m", "depth_pixels", "depth_refined")})
        assert _same(mine, child[s]), s
    assert any(rec["right"]["depth_refined"] for rec in child.values())
