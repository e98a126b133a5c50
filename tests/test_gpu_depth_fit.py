"""GPU: hm_depth_fit against the numpy rule of tests/depth_fit_rule.py where the vectors, the image borders, the per-workgroup
query slots and the wave sums can go wrong; its batch invariance and buffers; fit_rigid on the ellipsoid drawn by render_views.

The maps are BLOBS on a smooth depth field -- rectangles and discs of one id over a plane with bumps -- because a pixel needs
four neighbours of its own id to have a normal; every test asserts from the rule that its queries use at least 50 pixels.

Bounds.  sums and counts are integers: every comparison of them is exact equality.  solution is compared with the rule's solve
of the SAME integers within 64 * cond(M) * 2^-53 * max|x|, the backward-error bound of a 6 x 6 Cholesky solve, with
cond(M) <= 1e5 asserted on the inputs; the rms is one division and one square root of the same numbers: 2^-52 relative.  The
fitted ellipsoid's mean vertex error is at most 2 x HOST_END_MM (what the rule's loop reaches on its own renders,
tests/test_depth_fit_host.py) + 1 mm, one raw unit of the sensor, for the rim pixels the two renderers may draw differently."""
import os
import sys
import time

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import depth_eval_rule as DR  # noqa: E402
import depth_fit_rule as FR  # noqa: E402

from hamer_yolo_amd import lib as L  # noqa: E402
from hamer_yolo_amd import render  # noqa: E402
from hamer_yolo_amd.hamer.utils import depth_eval as DE  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
HOST_END_MM = 0.02                                                                    # tests/test_depth_fit_host.py measures and pins it
KW = dict(unit=0.001, gate_m=0.03, edge_m=0.005, reach_m=0.5, damping=0.02, lever_m=0.2, min_pixels=50)
RULE_KEYS = ("unit", "gate_m", "edge_m", "reach_m", "raw_range", "mask", "labels")


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def field(N, H, W, slope=1e-4, frame_step=0.0):
    """A smooth depth field: a tilted plane with bumps, float32; the sensor sees it up to 4 mm off, smoothly."""
    n, v, u = np.meshgrid(np.arange(N), np.arange(H), np.arange(W), indexing="ij")
    z = 0.5 + slope * u + slope * v + 0.003 * np.sin(u / 7.0) * np.cos(v / 5.0) + frame_step * n
    off = 0.004 * np.sin(u / 11.0 + v / 13.0 + n)
    return z.astype(np.float32), np.rint((z + off) * 1000.0).astype(np.uint16)


def rect(pid, n, v0, v1, u0, u1, i):
    pid[n, v0:v1, u0:u1] = i


def disc(pid, n, cv, cu, r, i):
    v, u = np.ogrid[:pid.shape[1], :pid.shape[2]]
    pid[n][(v - cv) ** 2 + (u - cu) ** 2 <= r * r] = i


def camera(H, W, N, f=600.0):
    return np.repeat(np.array([[f, f, (W - 1) / 2.0, (H - 1) / 2.0]]), N, 0)


def k_of(cams):
    K = np.zeros((len(cams), 3, 3))
    K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2], K[:, 2, 2] = cams[:, 0], cams[:, 1], cams[:, 2], cams[:, 3], 1.0
    return K


def pivots(Q, z=0.5):
    return np.array([[0.002 * q - 0.003, 0.001 * q, z + 0.01 * (q % 3)] for q in range(Q)], np.float64).reshape(Q, 3)


def check(got, depth, pid, sensor, mq, Q, cams, pv, min_used=50, solved=None, **kw):
    """``got`` (a depth_fit dict) equals the rule on the host arrays; returns (sums, counts, solution) of the rule."""
    rule = {k: v for k, v in kw.items() if k in RULE_KEYS}
    sums, counts = FR.fit(depth, pid, sensor, mq, Q, cams, pv, **rule)
    sol = FR.solve(sums, counts, kw["damping"], kw["lever_m"], kw["min_pixels"])
    gs, gc, gx = got["sums"].cpu().numpy(), got["counts"].cpu().numpy(), got["solution"].cpu().numpy()
    assert gs.dtype == np.int64 and gc.dtype == np.int64 and gx.dtype == np.float64
    assert gs.shape == (Q, 28) and gc.shape == (Q, 8) and gx.shape == (Q, 8)
    assert np.array_equal(gc, counts), (gc.tolist(), counts.tolist())
    assert np.array_equal(gs, sums), np.argwhere(gs != sums)[:8].tolist()
    assert (counts[:, 0] == counts[:, 1:7].sum(1)).all() and (counts[:, 7] == 0).all()
    if min_used:
        assert (counts[:, 6] >= min_used).all(), counts[:, 6].tolist()                # nothing passes by leaving everything out
    assert np.array_equal(gx[:, 7], sol[:, 7]) and (solved is None or sol[:, 7].tolist() == solved), (gx[:, 7], sol[:, 7])
    assert np.array_equal(np.isnan(gx[:, 6]), np.isnan(sol[:, 6])) and not np.isnan(gx[:, :6]).any()
    for q in range(Q):
        if not np.isnan(sol[q, 6]):
            assert abs(gx[q, 6] - sol[q, 6]) <= 2.0 ** -52 * sol[q, 6], (q, gx[q, 6], sol[q, 6])
        if sol[q, 7] == 0.0:
            assert gx[q, :6].tobytes() == np.zeros(6).tobytes()
            continue
        M, _ = FR.matrix(sums[q], counts[q, 6], kw["damping"], kw["lever_m"])
        cond = np.linalg.cond(M)
        assert cond <= 1e5, (q, cond)
        bound = 64.0 * cond * 2.0 ** -53 * np.abs(sol[q, :6]).max()
        assert (np.abs(gx[q, :6] - sol[q, :6]) <= bound).all(), (q, gx[q, :6].tolist(), sol[q, :6].tolist(), bound)
    return sums, counts, sol


def run(depth, pid, sensor, mq, Q, cams, pv, min_used=50, solved=None, **kw):
    args = dict(KW, **kw)
    mask, labels = args.pop("mask", None), args.pop("labels", None)
    got = DE.depth_fit(dev(depth), dev(pid), dev(sensor), mq, Q, k_of(cams), dev(pv), mask=dev(mask), labels=labels, **args)
    return got, check(got, depth, pid, sensor, mq, Q, cams, pv, min_used, solved, **dict(KW, **kw))


def abi(depth, pid, sensor, mq, Q, cams, pv, ws=None, out=None, extra=64, fill=0xA5, mask=None, labels=None, **kw):
    """hm_depth_fit itself on device tensors, the outputs and the workspace pre-filled with ``fill`` bytes unless given."""
    a = dict(KW, raw_range=(1, 65535), **kw)
    lib = L.load()
    N, H, W = pid.shape
    if out is None:
        out = {"sums": torch.full((Q, 28 * 8), fill, dtype=torch.uint8, device=DEV).view(torch.int64),
               "counts": torch.full((Q, 64), fill, dtype=torch.uint8, device=DEV).view(torch.int64),
               "solution": torch.full((Q, 64), fill, dtype=torch.uint8, device=DEV).view(torch.float64)}
    need = int(lib.hm_depth_fit_workspace_bytes(Q))
    if ws is None:
        ws = torch.full((need + extra,), fill, dtype=torch.uint8, device=DEV)
    before = ws[need:].clone()
    mqd = dev(np.asarray(mq, np.int32))
    L.check(lib.hm_depth_fit(L.ptr(depth), L.ptr(pid), L.ptr(sensor), L.ptr(mask), L.ptr(labels), N, H, W, L.ptr(mqd), len(mq), Q,
                             L.ptr(cams), L.ptr(pv), a["unit"], a["raw_range"][0], a["raw_range"][1], a["gate_m"], a["edge_m"],
                             a["reach_m"], a["damping"], a["lever_m"], a["min_pixels"], L.ptr(out["sums"]) if Q else None,
                             L.ptr(out["counts"]) if Q else None, L.ptr(out["solution"]) if Q else None, L.ptr(ws), ws.numel(),
                             L.current_stream()), "hm_depth_fit")
    torch.cuda.synchronize()
    assert torch.equal(ws[need:], before)                                             # nothing is written past what was asked for
    return out, ws


def same(a, b):
    return all(a[k].cpu().numpy().tobytes() == b[k].cpu().numpy().tobytes() for k in ("sums", "counts", "solution"))


def border_maps():
    """N = 2, 19 x 23: mesh 0 fills frame 0 -- it touches every border -- and the first rows of frame 1, so the last row of
    frame 0 sits over a row of its own id and nearly its own depth in the next frame, and every row's last pixel is followed by
    the next row's first of its own id within edge_m; mesh 1 is a disc cut by the right border of frame 1."""
    N, H, W = 2, 19, 23
    depth, sensor = field(N, H, W)
    pid = np.full((N, H, W), -1, np.int32)
    rect(pid, 0, 0, H, 0, W, 0)
    rect(pid, 1, 0, 7, 0, W, 0)
    disc(pid, 1, 13, 19, 6, 1)
    assert np.abs(np.diff(depth.reshape(-1).astype(np.float64)))[pid.reshape(-1)[:-1] == 0].max() < KW["edge_m"]   # wraps pass the depth test
    return np.where(pid >= 0, depth, np.float32(0)), pid, sensor, camera(H, W, N), pivots(2)


# ------------------------------------------------------------------ a: borders, row wrap and frame wrap
def test_borders_and_wraps():
    depth, pid, sensor, cams, pv = border_maps()
    _, (sums, counts, sol) = run(depth, pid, sensor, [0, 1], 2, cams, pv, solved=[1.0, 1.0])
    N, H, W = pid.shape
    # mesh 0: the only pixels with a normal are the interiors of its two rectangles
    assert counts[0, 4] == (pid == 0).sum() - (H - 2) * (W - 2) - 5 * (W - 2) and counts[0, 6] + counts[0, 5] == (H - 2) * (W - 2) + 5 * (W - 2)
    assert counts[1, 4] > 0 and counts[:, 3].sum() == 0


# ------------------------------------------------------------------ b: bases 1, 2 and 3 elements past a 16-byte boundary
def test_unaligned_bases():
    depth, pid, sensor, cams, pv = border_maps()
    n = pid.size
    assert n % 4 == 2 and (pid.shape[1] * pid.shape[2]) % 4 == 1
    ref = None
    for off in (0, 1, 2, 3):
        d, i, s = (torch.zeros(n + 8, dtype=t.dtype, device=DEV) for t in (dev(depth), dev(pid), dev(sensor)))
        i.fill_(0)                                                                     # mesh 0 before and behind the view: never read
        d[off:off + n], i[off:off + n], s[off:off + n] = dev(depth).reshape(-1), dev(pid).reshape(-1), dev(sensor).reshape(-1)
        d, i, s = (t[off:off + n].view(pid.shape) for t in (d, i, s))
        assert i.data_ptr() % 16 == 4 * off and i.is_contiguous()
        got = DE.depth_fit(d, i, s, [0, 1], 2, k_of(cams), dev(pv), **KW)
        check(got, depth, pid, sensor, [0, 1], 2, cams, pv, **KW)
        ref = ref or got
        assert same(ref, got)
    DE.release_fit_workspaces()


# ------------------------------------------------------------------ c: more than one workgroup, more queries than LDS slots
def big_maps():
    N, H, W = 3, 120, 160
    depth, sensor = field(N, H, W, slope=2e-5, frame_step=0.01)
    pid = np.full((N, H, W), -1, np.int32)
    for k in range(6):                                                                 # six queries inside the first workgroup's 32768 pixels
        rect(pid, 0, 5 + 38 * (k // 3), 40 + 38 * (k // 3), 4 + 52 * (k % 3), 50 + 52 * (k % 3), k)
    disc(pid, 0, 100, 80, 18, 6)
    disc(pid, 1, 85, 80, 30, 7)                                                        # pixel 32768 is row 84 of frame 1: two workgroups share it
    rect(pid, 1, 2, 30, 2, 158, 8)
    rect(pid, 2, 10, 110, 10, 150, 9)                                                  # 14000 pixels of one query
    disc(pid, 2, 60, 80, 20, 10)
    return np.where(pid >= 0, depth, np.float32(0)), pid, sensor, camera(H, W, N), pivots(11, 0.51)


def test_many_queries_and_workgroups():
    depth, pid, sensor, cams, pv = big_maps()
    assert pid.size > 32768 and len(np.unique(pid[0][pid[0] >= 0])) == 7
    _, (sums, counts, sol) = run(depth, pid, sensor, list(range(11)), 11, cams, pv, solved=[1.0] * 11)
    assert counts[9, 6] > 9000 and (np.abs(sums[:, :21]).max(1) > 2 ** 30).all()
    # the same maps as one query, and as two with the meshes interleaved
    run(depth, pid, sensor, [0] * 11, 1, cams, pv[:1], solved=[1.0])
    run(depth, pid, sensor, [k % 2 for k in range(11)], 2, cams, pv[:2], solved=[1.0, 1.0])
    DE.release_fit_workspaces()


# ------------------------------------------------------------------ d, e: mesh_query cases, masks, labels and the raw range
def test_mesh_query_masks_and_raw_range():
    depth, pid, sensor, cams, pv = big_maps()
    pid[0, 110:118, 100:150] = 17                                                      # an id past n_meshes
    depth[0, 110:118, 100:150] = 0.5
    mq = [0, 1, 0, -1, 2, 3, 2, 2, 1, 5, 5, 4]                                         # meshes share queries, mesh 3 counts for none,
    Q = 6                                                                              # mesh 11 (query 4) has no pixel
    _, (sums, counts, sol) = run(depth, pid, sensor, mq, Q, cams, pv[:Q], min_used=0, solved=[1.0, 1.0, 1.0, 1.0, 0.0, 1.0])
    assert counts[4].sum() == 0 and np.isnan(sol[4, 6]) and counts[:, 0].sum() == np.isin(pid, [0, 1, 2, 4, 5, 6, 7, 8, 9, 10]).sum()
    assert (counts[[0, 1, 2, 3, 5], 6] >= 50).all()
    _, (s1, c1, _) = run(depth, pid, sensor, mq, 3, cams, pv[:3], min_used=0)          # queries at or past Q are skipped
    assert np.array_equal(s1, sums[:3]) and np.array_equal(c1, counts[:3])
    run(depth, pid, sensor, [], 2, cams, pv[:2], min_used=0, solved=[0.0, 0.0])         # no mesh at all
    # e: a label image and the raw range
    rng = np.random.default_rng(5)
    mask = np.zeros(pid.shape, np.uint8)
    mask[:, :, :90], mask[:, :, 90:] = 3, 5
    mask[rng.random(pid.shape) < 0.02] = 0
    for labels in ([-2, -1, 3, 5, -2, 200], [3] * Q, [-2] * Q):
        _, (s2, c2, _) = run(depth, pid, sensor, mq, Q, cams, pv[:Q], min_used=0, mask=mask, labels=labels)
        if labels[0] == 3:
            assert c2[:, 1].sum() > 1000 and c2[:, 6].sum() >= 50
    assert np.array_equal(s2, sums) and np.array_equal(c2, counts)                    # -2 everywhere: no mask test
    lo, hi = int(np.percentile(sensor[pid >= 0], 30)), int(np.percentile(sensor[pid >= 0], 80))
    holes = sensor.copy()
    holes[rng.random(pid.shape) < 0.05] = 0
    _, (s3, c3, _) = run(depth, pid, holes, mq, Q, cams, pv[:Q], min_used=0, raw_range=(lo, hi))
    assert c3[:, 2].sum() > 1000 and c3[:, 6].sum() >= 50
    DE.release_fit_workspaces()


# ------------------------------------------------------------------ f, g: per-frame cameras, per-query pivots, the gate, a NaN
def test_cameras_pivots_gate_and_nan():
    depth, pid, sensor, cams, pv = big_maps()
    cams = np.array([[600.0, 590.0, 79.5, 59.5], [450.0, 470.0, 70.0, 66.0], [700.0, 710.0, 90.25, 50.75]])
    pv = pivots(11, 0.51)
    pv[9] = [0.0, 0.0, 1.2]                                                            # farther than reach_m from all its pixels
    solved = [1.0] * 11
    solved[9] = 0.0
    _, (sums, counts, sol) = run(depth, pid, sensor, list(range(11)), 11, cams, pv, min_used=0, solved=solved)
    assert counts[9, 6] == 0 and counts[9, 5] > 9000 and (sums[9] == 0).all() and (np.delete(counts[:, 6], 9) >= 50).all()
    one = FR.fit(depth, pid, sensor, list(range(11)), 11, camera(120, 160, 3), pv)[0]
    assert not np.array_equal(one[7], sums[7])                                         # the cameras matter
    # g: a band of the sensor 35 mm off is gated; a NaN or infinite depth is gated and takes its four neighbours' normals away
    far = sensor.copy()
    far[2, 40:60, :] += 35
    d2 = depth.copy()
    d2[1, 85, 80] = np.nan
    d2[0, 20, 20] = np.inf
    _, (s2, c2, _) = run(d2, pid, far, list(range(11)), 11, cams, pv, min_used=0)
    assert c2[9, 3] + c2[10, 3] == 20 * 140 and c2[10, 3] > 0 and counts[9, 3] == counts[10, 3] == 0
    for q in (0, 7):
        assert c2[q, 3] == counts[q, 3] + 1 and c2[q, 4] == counts[q, 4] + 4 and c2[q, 6] >= 50
    DE.release_fit_workspaces()


# ------------------------------------------------------------------ h: independence and exact sums
def test_independence_and_exact_sums():
    depth, pid, sensor, cams, pv = big_maps()
    Q = 11
    args = [dev(a) for a in (depth, pid, sensor)]
    whole = DE.depth_fit(*args, list(range(Q)), Q, k_of(cams), dev(pv), **KW)
    check(whole, depth, pid, sensor, list(range(Q)), Q, cams, pv, **KW)
    for q in range(Q):                                                                 # each query alone
        mq = [0 if k == q else -1 for k in range(Q)]
        alone = DE.depth_fit(*args, mq, 1, k_of(cams), dev(pv[q:q + 1]), **KW)
        assert same({k: v[q:q + 1] for k, v in whole.items()}, alone), q
    back = DE.depth_fit(*args, list(range(Q))[::-1], Q, k_of(cams), dev(pv[::-1]), **KW)
    assert same({k: v.flip(0) for k, v in back.items()}, whole)
    twice = DE.depth_fit(*[torch.cat([t, t]) for t in args], list(range(Q)), Q, k_of(np.concatenate([cams, cams])), dev(pv), **KW)
    assert torch.equal(twice["sums"], 2 * whole["sums"]) and torch.equal(twice["counts"], 2 * whole["counts"])
    assert same(whole, DE.depth_fit(*args, list(range(Q)), Q, k_of(cams), dev(pv), **KW))   # and run to run
    DE.release_fit_workspaces()


# ------------------------------------------------------------------ i: state left over from earlier calls
def test_buffers_and_leftover_state():
    depth, pid, sensor, cams, pv = border_maps()
    d, i, s, c, p = (dev(a) for a in (depth, pid, sensor, cams, pv))
    ref = DE.depth_fit(d, i, s, [0, 1], 2, k_of(cams), p, **KW)
    check(ref, depth, pid, sensor, [0, 1], 2, cams, pv, **KW)
    out, ws = abi(d, i, s, [0, 1], 2, c, p)                                            # 0xA5 in every output and the workspace beforehand
    assert same(out, ref)
    out2, _ = abi(d, i, s, [1, 0], 2, c, p, ws=ws, out=out)                            # a used workspace and stale outputs
    swapped = DE.depth_fit(d, i, s, [1, 0], 2, k_of(cams), p, **KW)
    assert same(out2, swapped) and not same(swapped, ref)
    out3, _ = abi(d, i, s, [0, 1], 2, c, p, extra=4096, fill=0xFF)                     # an oversized workspace
    assert same(out3, ref)
    need = int(L.load().hm_depth_fit_workspace_bytes(2))
    assert need == 2 * 36 * 8
    out4, ws4 = abi(d, i, s, [0, 1], 0, c, p, out={k: v.clone() for k, v in out3.items()}, extra=need)   # Q == 0: no launch
    assert same(out4, out3) and bool((ws4 == 0xA5).all())
    none = DE.depth_fit(d, i, s, [0, 1], 0, k_of(cams), p[:0].contiguous(), **KW)
    assert none["sums"].shape == (0, 28) and none["counts"].shape == (0, 8) and none["solution"].shape == (0, 8)
    DE.release_fit_workspaces()
    assert DE._fit_ws == {}


# ------------------------------------------------------------------ j: too few pixels, and a singular M
def test_not_solved():
    depth, pid, sensor, cams, pv = border_maps()
    _, (sums, counts, sol) = run(depth, pid, sensor, [0, 1], 2, cams, pv, min_pixels=int(1e6), solved=[0.0, 0.0])
    assert np.isfinite(sol[:, 6]).all()
    got, (sums, counts, sol) = run(depth, pid, sensor, [0, 1], 2, cams, pv, min_used=0, min_pixels=70, solved=[1.0, 0.0])
    assert 50 <= counts[1, 6] < 70
    # one flat fronto-parallel patch without damping: n = (0, 0, nz) exactly, so the third diagonal of the factorisation is 0
    N, H, W = 1, 40, 50
    flat = np.full((N, H, W), 0.5, np.float32)
    pid1 = np.zeros((N, H, W), np.int32)
    raw = np.full((N, H, W), 503, np.uint16)
    got, (sums, counts, sol) = run(flat, pid1, raw, [0], 1, camera(H, W, N), pivots(1), damping=0.0, solved=[0.0])
    assert counts[0, 6] == 38 * 48 and abs(sol[0, 6] - 0.003) < 1e-6 and sums[0, 20] > 0 and (sums[0, [2, 7, 11, 12, 13, 14]] == 0).all()
    assert not np.isnan(got["solution"].cpu().numpy()[0, :6]).any()
    run(flat, pid1, raw, [0], 1, camera(H, W, N), pivots(1), solved=[1.0])             # with damping the same patch is solved
    DE.release_fit_workspaces()


# ------------------------------------------------------------------ k: depth_fit and fit_rigid on the ellipsoid
SCENE = dict(H=240, W=320, K=np.array([[600.0, 0, 160.0], [0, 600.0, 120.0], [0, 0, 1.0]]), centre=np.array([0.03, -0.02, 0.5]),
             wall=1.5, unit=0.001, degrees=8.0, axis=(0.5, 0.7, 0.5), shift=(0.010, -0.008, 0.040))


def test_fit_rigid_on_the_ellipsoid(monkeypatch):
    v, f = DR.ellipsoid()
    H, W, K, unit, c = SCENE["H"], SCENE["W"], SCENE["K"], SCENE["unit"], SCENE["centre"]
    faces = torch.from_numpy(f).to(DEV)
    B = 2                                                                              # the second hand's frame measured nothing

    def gpu_render(placed):
        meshes = [{"frame": j, "vertices": torch.from_numpy(np.ascontiguousarray(placed[j])).to(DEV), "faces": faces} for j in range(len(placed))]
        r = render.render_views(H, W, K, meshes, outputs=("depth", "mesh_id"), views=B, device=DEV)
        return r["depth"].cpu().numpy(), r["mesh_id"].cpu().numpy()

    truth = np.repeat((v + c)[None], B, 0)
    depth, mid = gpu_render(truth)
    sensor = DR.sensor_from_depth(depth, unit, SCENE["wall"])
    sensor[1] = 0
    axis = np.asarray(SCENE["axis"]) / np.linalg.norm(SCENE["axis"])
    Re = FR.exp_so3(axis * np.radians(SCENE["degrees"]))
    verts = np.repeat((v @ Re.T)[None].astype(np.float32), B, 0)
    start = np.repeat((c + np.asarray(SCENE["shift"]))[None].astype(np.float32), B, 0)
    pivot = start.astype(np.float64)

    def err(p):
        return np.linalg.norm(p - truth, axis=2).mean(1) * 1e3

    # one depth_fit call on the GPU's render of the ray-refined hands equals the rule
    ray = DE.refine_cam_t(H, W, K, dev(verts), faces, dev(start), [0, 1], dev(sensor), unit=unit)
    cam_ray = ray["cam_t"].cpu().numpy()
    placed = verts.astype(np.float64) + cam_ray.astype(np.float64)[:, None, :]
    d1, m1 = gpu_render(placed)
    pv1 = pivot + (cam_ray.astype(np.float64) - start.astype(np.float64))
    kw = dict(unit=unit, gate_m=0.03, edge_m=0.005, reach_m=0.5, damping=1e-3, lever_m=0.05, min_pixels=200)
    got = DE.depth_fit(dev(d1), dev(m1), dev(sensor), [0, 1], 2, K, dev(pv1), unit=unit)
    _, counts, _ = check(got, d1, m1, sensor, [0, 1], 2, FR.cameras_of(K, B), pv1, min_used=0, solved=[1.0, 0.0], **kw)
    assert counts[0, 6] > 10000 and counts[1, 2] == counts[1, 0] > 10000

    args = (H, W, K, dev(verts), faces, dev(start), dev(pivot), [0, 1], dev(sensor))
    DE.fit_rigid(*args, unit=unit, iterations=1)                                       # warm: modules loaded, workspaces cached
    torch.cuda.synchronize()
    # the loops never wait for the GPU: half a second of earlier work on the stream is still running when fit_rigid returns
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    torch.cuda._sleep(1000000)
    t1.record()
    torch.cuda.synchronize()
    spin = int(1000000 * 500.0 / max(t0.elapsed_time(t1), 1e-3))                      # the spin count of half a second on this clock
    state = {}
    real = render.render_views

    def first_render(*a, **k):
        if not state:
            torch.cuda._sleep(spin)
            state["busy"] = torch.cuda.Event()
            state["busy"].record()
            state["t0"] = time.perf_counter()
        return real(*a, **k)

    monkeypatch.setattr(render, "render_views", first_render)
    got = DE.fit_rigid(*args, unit=unit)
    waited = state["busy"].query()
    print("fit_rigid: two ray and six rigid rounds enqueued in %.1f ms" % ((time.perf_counter() - state["t0"]) * 1e3))
    monkeypatch.setattr(render, "render_views", real)
    assert not waited
    out = {k: t.cpu().numpy() for k, t in got.items()}
    e_ray, e_fit = err(placed), err(out["placed"])
    print("mean vertex error in mm: start", err(verts.astype(np.float64) + start[:, None]), "ray only", e_ray, "rigid", e_fit,
          "rms", out["rms"], "used", out["used"])
    assert e_fit[0] <= 2 * HOST_END_MM + 1.0 and e_fit[0] < e_ray[0]
    assert out["updated"].tolist() == [True, False] and out["fitted"].tolist() == [True, False] and out["used"][0] > 10000
    assert out["cam_t"].dtype == np.float32 and out["cam_t"][1].tobytes() == start[1].tobytes()
    assert out["rotation"][1].tobytes() == np.eye(3).tobytes() and out["pivot"][1].tobytes() == pivot[1].tobytes()
    # what is returned is consistent: placed = rotation (vertices + ray cam_t - ray pivot) + pivot, cam_t = ray cam_t + pivot's shift
    again = np.einsum("ij,vj->vi", out["rotation"][0], placed[0] - pv1[0]) + out["pivot"][0]
    assert np.abs(again - out["placed"][0]).max() <= 1e-12
    assert np.abs(out["cam_t"][0] - (cam_ray[0].astype(np.float64) + out["pivot"][0] - pv1[0])).max() <= 1e-7
    assert np.abs(out["rotation"][0] @ out["rotation"][0].T - np.eye(3)).max() <= 1e-13
    # steps over the caps are not applied: every hand keeps its bytes
    capped = DE.fit_rigid(*args, unit=unit, ray_iterations=0, max_rot_rad=1e-9)
    assert capped["cam_t"].cpu().numpy().tobytes() == start.tobytes() and not bool(capped["updated"].any())
    assert capped["rotation"].cpu().numpy().tobytes() == np.repeat(np.eye(3)[None], B, 0).tobytes()
    render.release_workspaces()
    DE.release_workspaces()
    DE.release_fit_workspaces()


# ------------------------------------------------------------------ the contraction map of the host tests
def test_contraction_map():
    depth, pid, sensor, cams, pv, unit, plain, fused = FR.contraction_case()
    _, (sums, counts, _) = run(depth, pid, sensor, [0], 1, cams, pv, unit=unit, solved=[1.0])
    assert sums[0, 26] == counts[0, 6] * plain != counts[0, 6] * fused
    DE.release_fit_workspaces()


# ------------------------------------------------------------------ l: a folder round trip on a synthetic MANO model
class _Cfg:
    ckpt_path = "synthetic:0"
    model_cfg = None
    use_onnx = False
    onnx_path = None


FH, FW = 192, 256
FK = np.array([[300.0, 0.0, 128.0], [0.0, 300.0, 96.0], [0.0, 0.0, 1.0]])
ROUND_TRIP_M = 2e-4                                                                    # tests/test_gpu_api.py: a record's OBJ against its vertices


def _same(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    if isinstance(a, float) and np.isnan(a):
        return isinstance(b, float) and np.isnan(b)
    return type(a) is type(b) and a == b


def test_folder_round_trip(tmp_path):
    from hamer_yolo_amd import evaluate_depth as ED
    from hamer_yolo_amd import infer
    hi = infer.hamer_inference(_Cfg)
    npy_dir, depth_dir, ray_dir, ray2_dir, fit_dir = (tmp_path / d for d in ("npy", "depth", "ray", "ray2", "fit"))
    npy_dir.mkdir(); depth_dir.mkdir()
    rng = np.random.default_rng(21)
    sides = {"b0": ("right", "left"), "b1": ("right",), "b2": ("left",), "b3": ("right",)}
    faces = torch.as_tensor(np.asarray(hi.mano.faces, np.int32), device=DEV)
    truth = {}
    for stem, ts in sides.items():
        rec = {"right": None, "left": None}
        for t in ts:
            pg, ph = rng.normal(0, 0.3, 3).astype(np.float32), rng.normal(0, 0.15, 45).astype(np.float32)
            rec[t] = {"betas": rng.normal(0, 0.5, 10).astype(np.float32), "theta": np.concatenate([pg, ph]), "pose_hand": ph,
                      "pose_global": pg, "cam_t": np.array([-0.12 if t == "right" else 0.12, 0.0, 0.7], np.float32), "is_right": t == "right"}
        truth[stem] = rec
        hands = [rec[t] for t in ts]
        verts = render.camera_vertices(hi, hands)
        meshes = [{"frame": 0, "vertices": verts[j], "faces": faces} for j in range(len(hands))]
        depth = render.render_views(FH, FW, FK, meshes, outputs=("depth",), views=1, device=DEV)["depth"][0].cpu().numpy()
        if stem != "b3":                                                               # b3 is given no depth map
            np.save(depth_dir / f"{stem}.npy", DR.sensor_from_depth(depth, 0.001, 1.5))
        # the prediction: 4 % too near, turned by 5 degrees about its wrist, a few millimetres to the side
        pred = {"right": None, "left": None}
        for t in ts:
            axis = rng.normal(size=3)
            w = axis / np.linalg.norm(axis) * np.radians(5.0)
            pg = ED.fold_rotation(rec[t]["pose_global"], FR.exp_so3(w), True).astype(np.float32)   # applied on MANO's side, either hand
            cam_t = (rec[t]["cam_t"].astype(np.float64) / 1.04 + np.array([0.004, -0.003, 0.0])).astype(np.float32)
            pred[t] = dict(rec[t], pose_global=pg, theta=np.concatenate([pg, rec[t]["pose_hand"]]), cam_t=cam_t)
        np.save(npy_dir / f"{stem}.npy", pred)

    def placed_of(rec_hands):
        return render.camera_vertices(hi, rec_hands).cpu().numpy().astype(np.float64)

    # mode='ray' writes what refine_folder always wrote: the records of refine_cam_t folded by _refined_record
    st_ray = ED.refine_folder(str(npy_dir), str(depth_dir), str(ray_dir), hi, FK)
    st_ray2 = ED.refine_folder(str(npy_dir), str(depth_dir), str(ray2_dir), hi, FK, mode="ray")
    assert st_ray == st_ray2 == {"records": 4, "hands": 5, "refined": 4, "skipped": ["b3"], "n_skipped": 1}
    st = ED.refine_folder(str(npy_dir), str(depth_dir), str(fit_dir), hi, FK, mode="rigid")
    assert st == dict(st_ray, fitted=4) and DE._fit_ws == {} and DE._ws == {}
    e_pred, e_ray, e_fit = [], [], []
    for stem, ts in sides.items():
        before = np.load(npy_dir / f"{stem}.npy", allow_pickle=True).item()
        ray, ray2, fit = (np.load(d / f"{stem}.npy", allow_pickle=True).item() for d in (ray_dir, ray2_dir, fit_dir))
        assert _same(ray, ray2)
        hands = [before[t] for t in ts]
        sign = torch.tensor([[1.0, 1.0, 1.0] if h["is_right"] else [-1.0, 1.0, 1.0] for h in hands], device=DEV)
        joints, verts = infer.mano_hand_joints_vertices(hi, hands)
        cam_t = torch.tensor(np.stack([h["cam_t"] for h in hands]), device=DEV)
        if stem != "b3":
            sensor = dev(np.load(depth_dir / f"{stem}.npy")[None])
            want = DE.refine_cam_t(FH, FW, FK[None], verts * sign[:, None, :], faces, cam_t, [0] * len(hands), sensor, unit=0.001)
            moved = {t: tuple(want[k].cpu().numpy()[j] for k in ("cam_t", "median", "valid", "updated")) for j, t in enumerate(ts)}
            assert _same(ray, ED._refined_record(before, moved))
            pivot = (joints[:, 0, :] * sign).to(torch.float64) + cam_t.to(torch.float64)
            r = DE.fit_rigid(FH, FW, FK[None], verts * sign[:, None, :], faces, cam_t, pivot, [0] * len(hands), sensor, unit=0.001)
            placed = r["placed"].cpu().numpy()
        else:
            assert _same(ray, ED._refined_record(before, {}))
        got = placed_of([fit[t] for t in ts])
        for j, t in enumerate(ts):
            a, b = fit[t], before[t]
            assert set(a) == set(b) | set(ED.NEW_KEYS) | set(ED.FIT_KEYS)
            assert all(_same(a[k], b[k]) for k in b if k not in ("cam_t", "pose_global", "theta"))
            assert _same(a["cam_t_unrefined"], b["cam_t"]) and _same(a["pose_global_unrefined"], b["pose_global"])
            assert a["pose_global"].dtype == np.float32 and a["theta"].dtype == np.float32 and np.array_equal(a["theta"][:3], a["pose_global"])
            assert np.array_equal(a["theta"][3:], b["theta"][3:])
            if stem == "b3":
                assert all(_same(a[k], b[k]) for k in b) and a["depth_fit"] is False and a["depth_fit_pixels"] == 0 and np.isnan(a["depth_fit_rms_m"])
                continue
            # the record, run through MANO again, is the mesh fit_rigid placed
            worst = np.abs(got[j] - placed[j]).max()
            true_v = placed_of([truth[stem][t]])[0]
            errs = [np.linalg.norm(v - true_v, axis=1).mean() * 1e3 for v in (placed_of([b])[0], placed_of([ray[t]])[0], got[j])]
            print(stem, t, "round trip %.2e m; mean vertex error in mm: predicted %.2f, ray %.2f, rigid %.2f; rms %.2e m over %d pixels" %
                  (worst, *errs, a["depth_fit_rms_m"], a["depth_fit_pixels"]))
            assert worst <= ROUND_TRIP_M
            assert a["depth_fit"] is True and a["depth_refined"] is True and a["depth_fit_pixels"] >= 200 and np.isfinite(a["depth_fit_rms_m"])
            assert errs[2] < errs[1] < errs[0]                                         # rigid ends below ray-only, hand by hand
            e_pred.append(errs[0]); e_ray.append(errs[1]); e_fit.append(errs[2])
    assert sum(e_fit) < sum(e_ray) < sum(e_pred)
    render.release_workspaces()
