"""GPU: hm_mask_fit against the numpy rule of tests/mask_fit_rule.py at the smallest shapes where the words, the borders and the
disc can go wrong; its batch invariance, buffers and argument errors; fit_contour on the ellipsoid drawn by render_views; the
drivers.

Shapes.  W = 70 and 130 with H = 40: rows end inside a word and a disc spans three words, and H = 40 is more than one tile of 32
rows; W = 64 with H = 3; radius 0, 1, 5 and 64 (at 64 the disc is wider than the W = 70 image); blobs cut by every border plus
set pixels in the first and last row and column; the tie shapes of the host test; a comb of one-pixel teeth at W = 130 whose
5000 boundary pixels of one query fill several waves of several workgroups.

Bounds.  sums and counts are integers: every comparison of them is exact equality.  solution is compared with the rule's solve of
the SAME integers within BOUND_C * cond(M) * 2^-53 * max|x| (tests/test_mask_fit_host.py derives BOUND_C for n = 4), with cond(M)
<= COND_MAX asserted on the inputs; the rms is one division and one square root of the same numbers: 2^-52 relative.  The fitted
ellipsoid ends at J >= HOST_END_J - 0.02 and a mean vertex error <= 2 x HOST_END_MM + the length one pixel spans at the hand's
depth (0.5 m / 600 = 0.83 mm), for the rim pixels the two renderers may draw differently."""
import os
import sys
import time

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mask_eval_rule as ER  # noqa: E402
import mask_fit_rule as MR  # noqa: E402
import test_mask_fit_host as TH  # noqa: E402

from hamer_yolo_amd import lib as L  # noqa: E402
from hamer_yolo_amd import render  # noqa: E402
from hamer_yolo_amd.hamer.utils import mask_eval as ME  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
KW = dict(radius=5, reach_px=4096, directions=3, damping=1e-3, lever_px=50.0, min_pixels=30)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def scene(H, W, seed, N=2):
    """pred_id with the ids 0..3 on blobs cut by the borders, a label image with 3 and 5, and set pixels in the first and last
    row and column of both."""
    pid = np.full((N, H, W), -1, np.int32)
    mask = np.zeros((N, H, W), np.uint8)
    for n in range(N):
        for i in range(4):
            pid[n][ER.blobs(H, W, seed + 10 * n + i, n=2)] = i
        mask[n][ER.blobs(H, W, seed + 50 + n, n=3)] = 3
        mask[n][ER.blobs(H, W, seed + 60 + n, n=1)] = 5
    pid[0, 0, 2:9], pid[0, H - 1, W - 9:], pid[0, H // 2:, 0], pid[0, :H // 2, W - 1] = 0, 1, 2, 0
    mask[0, 0, 5:12], mask[0, H - 1, :7], mask[0, 1:H // 2, 0], mask[0, H // 3:, W - 1] = 3, 3, 3, 3
    return pid, mask


def queries_of(pid, mask):
    """Queries on both frames, three on frame 0 with different id ranges, an empty id range, a label that is in no pixel,
    label -1, and frames outside the batch.  A centre is the rounded centroid of its query's pred and gt pixels, which keeps M
    well conditioned; the centre of query 1 lies left of the image, at a negative x."""
    q = [(0, 0, 1, 3), (0, 1, 3, 3), (0, 0, 4, -1), (1, 0, 2, 5), (1, 2, 4, 3), (0, 2, 2, 3), (1, 0, 4, 9), (2, 0, 1, 3), (-1, 0, 4, 3)]
    c = []
    for k, qu in enumerate(q):
        if not 0 <= qu[0] < len(pid):
            c.append((1, 2))
            continue
        pred, gt = ER.query_images(pid, mask, qu)
        ys, xs = np.nonzero(pred | gt)
        c.append((int(np.rint(xs.mean())), int(np.rint(ys.mean()))) if len(ys) else (3, 3))
    c[1] = (-3, c[1][1])
    return np.array(q, np.int32), np.array(c, np.int32)


def check(got, pid, mask, q, c, **kw):
    """``got`` (a mask_fit dict) equals the rule on the host arrays; returns (sums, counts, solution) of the rule."""
    Q = len(q)
    sums, counts = MR.fit(pid, mask, q, c, kw["radius"], kw["reach_px"], kw["directions"])
    sol = MR.solve(sums, counts, kw["damping"], kw["lever_px"], kw["min_pixels"])
    gs, gc, gx = got["sums"].cpu().numpy(), got["counts"].cpu().numpy(), got["solution"].cpu().numpy()
    assert gs.dtype == np.int64 and gc.dtype == np.int64 and gx.dtype == np.float64
    assert gs.shape == (Q, 18) and gc.shape == (Q, 2, 6) and gx.shape == (Q, 8)
    assert np.array_equal(gc, counts), (gc.tolist(), counts.tolist())
    assert np.array_equal(gs, sums), np.argwhere(gs != sums)[:8].tolist()
    assert not np.isnan(gx).any() and np.array_equal(gx[:, 5], sol[:, 5]) and (gx[:, 6:] == 0).all()
    for k in range(Q):
        assert abs(gx[k, 4] - sol[k, 4]) <= 2.0 ** -52 * sol[k, 4], (k, gx[k, 4], sol[k, 4])
        if sol[k, 5] == 0.0:
            assert gx[k, :4].tobytes() == np.zeros(4).tobytes()
            continue
        M, _ = MR.matrix(sums[k], counts[k], kw["damping"], kw["lever_px"])
        cond = np.linalg.cond(M)
        assert cond <= TH.COND_MAX, (k, cond)
        bound = TH.BOUND_C * cond * 2.0 ** -53 * np.abs(sol[k, :4]).max()
        assert (np.abs(gx[k, :4] - sol[k, :4]) <= bound).all(), (k, gx[k, :4].tolist(), sol[k, :4].tolist(), bound)
    return sums, counts, sol


def run(pid, mask, q, c, **kw):
    a = dict(KW, **kw)
    got = ME.mask_fit(dev(pid), dev(mask), dev(np.asarray(q, np.int32).reshape(-1, 4)), dev(np.asarray(c, np.int32).reshape(-1, 2)), **a)
    return got, check(got, pid, mask, q, c, **a)


def same(a, b):
    return all(a[k].cpu().numpy().tobytes() == b[k].cpu().numpy().tobytes() for k in ("sums", "counts", "solution"))


# ------------------------------------------------------------------ a: words, borders, discs, directions, query kinds
@pytest.mark.parametrize("H,W", [(40, 70), (40, 130), (3, 64)])
def test_shapes_radii_and_query_kinds(H, W):
    pid, mask = scene(H, W, seed=H + W)
    q, c = queries_of(pid, mask)
    for radius, directions in ((0, 3), (1, 1), (5, 3), (5, 2), (64, 3)):
        _, (sums, counts, sol) = run(pid, mask, q, c, radius=radius, directions=directions, min_pixels=5)
        assert (counts[5:, :, 1:3] == 0).all() and (sums[5:] == 0).all() and (sol[5:] == 0).all()      # nothing to match there
        assert (counts[7:] == 0).all()                                                 # frames outside the batch: not read
        if directions & 1:                                                             # a label in no pixel: all of pred is unmatched
            assert counts[6, 0, 0] > 0 and counts[6, 0, 0] == counts[6, 0, 3] and counts[6, 1].sum() == 0
        assert counts[5, 0].sum() == 0                                                 # an empty id range has no pred boundary
        if radius >= 5 and H > 3:
            assert (counts[[0, 1, 2, 4], :, 1].sum(1) > 20).all() and sol[:3, 5].tolist() == [1.0] * 3
        if radius == 64 and W <= 70:
            assert counts[:5, :, 3].sum() == 0                                         # the disc is wider than the image: all matched
        if radius == 0:
            assert (counts[:, :, 1] == 0).all() and (sums[:, :15] == 0).all()          # only anchors
    _, (sums, counts, _) = run(pid, mask, q, c, radius=5, reach_px=12)
    assert (counts[[0, 1, 2, 4], :, 4].sum(1) > 5).all() and counts[:5, :, 1].sum() > 20
    ME.release_fit_workspaces()


# ------------------------------------------------------------------ b: ties
def test_tie_shapes():
    shapes = MR.tie_shapes()
    pid = np.stack([np.where(p, 0, -1).astype(np.int32) for p, _ in shapes])
    mask = np.stack([g.astype(np.uint8) * 3 for _, g in shapes])
    q = [(n, 0, 1, 3) for n in range(3)]
    c = [(5, 4)] * 3
    for directions in (1, 2, 3):
        _, (sums, counts, _) = run(pid, mask, q, c, radius=6, directions=directions, min_pixels=1)
    # the pixel at the centre moves by (-3, 0), (0, -3), (-3, -3): with u = 0 its row is (0, 0, dx, dy) and it alone has d2 = 9 / 18
    for n, (pred, gt) in enumerate(shapes):
        p = MR.pixels(pred, gt, (5, 4), 6, 4096, 1)
        k = int(np.nonzero((p["yx"] == (4, 5)).all(1))[0][0])
        assert tuple(p["d"][k].tolist()) == [(-3, 0), (0, -3), (-3, -3)][n]
    ME.release_fit_workspaces()


# ------------------------------------------------------------------ c: many boundary pixels in one query
def test_comb_fills_waves_and_workgroups():
    H, W = 40, 130
    pred = np.zeros((H, W), bool)
    pred[1::2, 1::2] = True                                                            # one-pixel teeth: every pixel but the last row / column is boundary
    gt = ER.blobs(H, W, 77, n=4)
    pid, mask = np.where(pred, 0, -1).astype(np.int32)[None], gt.astype(np.uint8)[None] * 3
    for radius, directions in ((5, 3), (64, 1)):
        _, (sums, counts, sol) = run(pid, mask, [(0, 0, 1, 3)], [(60, 20)], radius=radius, directions=directions)
        assert counts[0, 0, 0] >= 5000 and sol[0, 5] == 1.0
        if radius == 64:
            assert counts[0, 0, 1] + counts[0, 0, 2] == counts[0, 0, 0] and np.abs(sums[0, :10]).max() > 2 ** 32
    ME.release_fit_workspaces()


# ------------------------------------------------------------------ d: batch invariance
def test_batch_invariance():
    H, W = 40, 130
    pid, mask = scene(H, W, seed=H + W)
    q, c = queries_of(pid, mask)
    args = (dev(pid), dev(mask))
    whole = ME.mask_fit(*args, dev(q), dev(c), **KW)
    check(whole, pid, mask, q, c, **KW)
    for k in (0, 2, 4):
        alone = ME.mask_fit(*args, dev(q[k:k + 1]), dev(c[k:k + 1]), **KW)
        assert same({n: v[k:k + 1] for n, v in whole.items()}, alone), k
    order = np.array([3, 7, 1, 8, 6, 0, 5, 2, 4])                                      # query 0 as query 5 of 9
    mixed = ME.mask_fit(*args, dev(q[order]), dev(c[order]), **KW)
    assert same({n: v[dev(order)] for n, v in whole.items()}, mixed)
    assert same(whole, ME.mask_fit(*args, dev(q), dev(c), **KW))                       # and run to run
    ME.release_fit_workspaces()


# ------------------------------------------------------------------ e: buffers, Q == 0
def abi(pid, mask, q, c, ws=None, out=None, extra=64, fill=0xA5, **kw):
    """hm_mask_fit itself on device tensors, the outputs and the workspace pre-filled with ``fill`` bytes unless given."""
    a = dict(KW, **kw)
    lib = L.load()
    N, H, W = pid.shape
    Q = len(q)
    if out is None:
        out = {"sums": torch.full((max(Q, 1), 18 * 8), fill, dtype=torch.uint8, device=DEV).view(torch.int64),
               "counts": torch.full((max(Q, 1), 12 * 8), fill, dtype=torch.uint8, device=DEV).view(torch.int64).view(-1, 2, 6),
               "solution": torch.full((max(Q, 1), 64), fill, dtype=torch.uint8, device=DEV).view(torch.float64)}
    need = int(lib.hm_mask_fit_workspace_bytes(Q, H, W, a["radius"]))
    if ws is None:
        ws = torch.full((need + extra,), fill, dtype=torch.uint8, device=DEV)
    before = ws[need:].clone()
    L.check(lib.hm_mask_fit(L.ptr(pid), L.ptr(mask), N, H, W, L.ptr(q) if Q else None, Q, L.ptr(c) if Q else None, a["radius"],
                            a["reach_px"], a["directions"], a["damping"], a["lever_px"], a["min_pixels"], L.ptr(out["sums"]),
                            L.ptr(out["counts"]), L.ptr(out["solution"]), L.ptr(ws), ws.numel(), L.current_stream()), "hm_mask_fit")
    torch.cuda.synchronize()
    assert torch.equal(ws[need:], before)                                             # nothing is written past what was asked for
    return out, ws


def test_buffers_and_leftover_state():
    H, W = 40, 70
    pid, mask = scene(H, W, seed=9)
    q, c = queries_of(pid, mask)
    d_pid, d_mask, d_q, d_c = dev(pid), dev(mask), dev(q), dev(c)
    ref = ME.mask_fit(d_pid, d_mask, d_q, d_c, **KW)
    check(ref, pid, mask, q, c, **KW)
    out, ws = abi(d_pid, d_mask, d_q, d_c)                                             # 0xA5 in every output and the workspace beforehand
    assert same(out, ref)
    flipped = dev(q[::-1].copy()), dev(c[::-1].copy())
    out2, _ = abi(d_pid, d_mask, *flipped, ws=ws, out=out)                             # a used workspace and stale outputs
    assert same(out2, {k: v.flip(0) for k, v in ref.items()})
    out3, _ = abi(d_pid, d_mask, d_q, d_c, extra=4096, fill=0xFF)                      # an oversized workspace
    assert same(out3, ref)
    assert int(L.load().hm_mask_fit_workspace_bytes(len(q), H, W, 5)) == len(q) * (2 * H * 2 + 32) * 8
    keep = {k: v.clone() for k, v in out3.items()}
    out4, ws4 = abi(d_pid, d_mask, d_q[:0], d_c[:0], out=out3, extra=0)                # Q == 0: no launch, nothing is touched
    assert same(out4, keep) and bool((ws4 == 0xA5).all())
    none = ME.mask_fit(d_pid, d_mask, [], [], **KW)
    assert none["sums"].shape == (0, 18) and none["counts"].shape == (0, 2, 6) and none["solution"].shape == (0, 8)
    ME.release_fit_workspaces()
    assert ME._fit_ws == {}


@pytest.mark.parametrize("H,W", [(3, 64), (37, 53), (70, 131)])
def test_both_entry_points_write_the_same_boundary_maps(H, W):
    """hm_mask_score and hm_mask_fit leave the same words at the head of their workspaces, each pre-filled with 0xA5: the
    boundary maps of the rule, 64 pixels per word, zero bits at or past W."""
    import test_gpu_mask_eval as GE
    gt = ER.blobs(H, W, 6)
    pid = np.where(ER.blobs(H, W, 5), 0, -1).astype(np.int32)[None]
    mask = np.where(gt, 3, 0).astype(np.uint8)[None]
    mask[0][ER.blobs(H, W, 7, n=1) & ~gt] = 5                                          # label -1 is more than label 3
    q = np.array([(0, 0, 1, 3), (0, 0, 1, -1)], np.int32)
    d_pid, d_mask = dev(pid), dev(mask)
    _, ws_score = GE.abi(d_pid, d_mask, q, KW["radius"])
    _, ws_fit = abi(d_pid, d_mask, dev(q), dev(np.array([(W // 2, H // 2)] * 2, np.int32)))
    words = (W + 63) // 64
    n = len(q) * 2 * H * words
    got_score, got_fit = (w.cpu().numpy()[:n * 8].view(np.uint64).reshape(len(q), 2, H, words) for w in (ws_score, ws_fit))
    want = np.zeros((len(q), 2, H, words * 64), bool)
    for k, qu in enumerate(q):
        for side, image in enumerate(ER.query_images(pid, mask, qu)):
            want[k, side, :, :W] = ER.bmap(image)
    want = np.packbits(want, axis=-1, bitorder="little").view(np.uint64)
    assert want[0].any() and not np.array_equal(want[0, 1], want[1, 1])
    assert np.array_equal(got_score, got_fit)
    assert np.array_equal(got_score, want), np.argwhere(got_score != want)[:8].tolist()


def test_argument_errors_with_real_buffers():
    """Every error the header lists, now over real device buffers: HM_ERR_ARG, and the outputs keep their bytes."""
    H, W = 37, 53
    pid, mask = scene(H, W, seed=3)
    q, c = queries_of(pid, mask)
    lib = L.load()
    buf = dict(pred_id=dev(pid), mask=dev(mask), queries=dev(q[:3]), centre=dev(c[:3]),
               sums=torch.full((3, 18), 7, dtype=torch.int64, device=DEV), counts=torch.full((3, 12), 7, dtype=torch.int64, device=DEV),
               solution=torch.full((3, 8), 7.0, dtype=torch.float64, device=DEV),
               workspace=torch.zeros(int(lib.hm_mask_fit_workspace_bytes(3, H, W, 5)) // 8 + 8, dtype=torch.int64, device=DEV))
    for kw, word in TH.ARG_CASES:
        a = dict(N=2, H=H, W=W, Q=3, radius=5, reach_px=4096, directions=3, damping=1e-3, lever_px=50.0, min_pixels=30,
                 workspace_bytes=buf["workspace"].numel() * 8, stream=L.current_stream())
        a.update({k: L.ptr(v) for k, v in buf.items()})
        for k, v in kw.items():
            a[k] = (None if v is None else a[k] + (v & 0xF)) if k in buf else v        # the made-up addresses' misalignment, on real ones
        rc = lib.hm_mask_fit(*[a[k] for k in TH.ORDER])
        msg = lib.hm_last_error_string().decode()
        assert rc == -1 and "hm_mask_fit" in msg and word in msg, (kw, rc, msg)
    torch.cuda.synchronize()
    assert bool((buf["sums"] == 7).all()) and bool((buf["counts"] == 7).all()) and bool((buf["solution"] == 7.0).all())
    with pytest.raises(ValueError, match="frame"):
        ME.mask_fit(buf["pred_id"], buf["mask"], [(2, 0, 1, 3)], [(0, 0)], **KW)        # a sequence of queries is checked on the host
    with pytest.raises(ValueError, match="centres"):
        ME.mask_fit(buf["pred_id"], buf["mask"], [(0, 0, 1, 3)], [(0, 0), (1, 1)], **KW)
    for bad in (dict(radius=65), dict(reach_px=0), dict(directions=0), dict(damping=-1.0), dict(lever_px=0.0), dict(min_pixels=0)):
        with pytest.raises(ValueError, match="expected"):
            ME.mask_fit(buf["pred_id"], buf["mask"], [(0, 0, 1, 3)], [(0, 0)], **dict(KW, **bad))


# ------------------------------------------------------------------ f: fit_contour on the ellipsoid
def test_fit_contour_on_the_ellipsoid(monkeypatch):
    v, f, truth, verts, start = TH.ellipsoid_scene()
    S = TH.SCENE
    H, W, K = S["H"], S["W"], S["K"]
    faces = torch.from_numpy(f).to(DEV)
    B = 3                                                                              # hand 1's frame has an empty mask; hand 2 shares frame 0 and its label

    def gpu_render(placed, views):
        meshes = [{"frame": j % views, "vertices": torch.from_numpy(np.ascontiguousarray(placed[j])).to(DEV), "faces": faces} for j in range(len(placed))]
        return render.render_views(H, W, K, meshes, outputs=("mesh_id",), views=views, device=DEV)["mesh_id"].cpu().numpy()

    mask = np.zeros((2, H, W), np.uint8)
    mask[0] = (gpu_render(truth.astype(np.float32), 1)[0] >= 0) * S["label"]
    one = dict(H=H, W=W, K=K, vertices=dev(verts), faces=faces, cam_t=dev(start), pivot=dev(start.astype(np.float64)), frame_index=[0],
               mask=dev(mask), labels=[S["label"]])
    # one mask_fit call on the GPU's render of the start equals the rule
    mid = gpu_render(verts.astype(np.float64) + start[:, None], 2)
    centre = MR.centre_of(MR.project(np.array([[600.0, 600.0, 160.0, 120.0]]), [0], start.astype(np.float64)))
    got = ME.mask_fit(dev(mid), dev(mask), [(0, 0, 1, 3)], centre, radius=S["radius"])
    _, counts, sol = check(got, mid, mask, [(0, 0, 1, 3)], centre, **dict(KW, radius=S["radius"]))
    assert counts[0, :, 1].sum() > 500 and sol[0, 5] == 1.0

    ME.fit_contour(**one, rounds=1, radius=S["radius"])                                # warm: modules loaded, workspaces cached
    torch.cuda.synchronize()
    # the loop never waits for the GPU: half a second of earlier work on the stream is still running when fit_contour returns
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
    got = ME.fit_contour(**one, radius=S["radius"])
    waited = state["busy"].query()
    print("fit_contour: six rounds enqueued in %.1f ms" % ((time.perf_counter() - state["t0"]) * 1e3))
    monkeypatch.setattr(render, "render_views", real)
    assert not waited
    out = {k: t.cpu().numpy() for k, t in got.items()}
    J = ER.jf(ER.counts(gpu_render(out["placed"], 1)[0] >= 0, mask[0] == S["label"], 4))[0]
    err = float(np.linalg.norm(out["placed"] - truth, axis=2).mean() * 1e3)
    print("fit_contour on the ellipsoid: J %.5f, mean vertex error %.3f mm, rms %.3f px over %d pixels" % (J, err, out["rms"][0], out["pixels"][0]))
    assert J >= TH.HOST_END_J - 0.02
    assert err <= 2 * TH.HOST_END_MM + 0.5 / 600.0 * 1e3
    assert out["fitted"].tolist() == [True] and out["pixels"][0] > 500 and out["cam_t"].dtype == np.float32
    p0 = start.astype(np.float64)
    again = np.einsum("ij,vj->vi", out["rotation"][0], verts[0].astype(np.float64)) + out["pivot"][0]
    assert np.abs(again - out["placed"][0]).max() <= 1e-12 and np.abs(out["cam_t"][0] - (p0[0] + out["pivot"][0] - p0[0])).max() <= 1e-7
    assert np.abs(out["rotation"][0] @ out["rotation"][0].T - np.eye(3)).max() <= 1e-13
    # three hands: hand 1 looks at an empty mask and keeps its bytes; hands 0 and 2 lie side by side in frame 0 under one label
    # -- the mask's contour is their union -- and are fitted pred -> mask only
    off = np.array([-0.11, 0.0, 0.0])
    mask3 = mask.copy()
    mask3[0] = (gpu_render(np.concatenate([truth, truth + off]).astype(np.float32), 1)[0] >= 0) * S["label"]
    start3 = np.concatenate([start, start, (start.astype(np.float64) + off * S["depth"]).astype(np.float32)])   # as far off in pixels as hand 0
    truth3 = np.concatenate([truth, truth, truth + off])
    three = ME.fit_contour(H, W, K, dev(np.repeat(verts, B, 0)), faces, dev(start3), dev(start3.astype(np.float64)), [0, 1, 0],
                           dev(mask3), [S["label"]] * B, radius=S["radius"])
    t3 = {k: t.cpu().numpy() for k, t in three.items()}
    e0 = np.linalg.norm(np.repeat(verts, B, 0).astype(np.float64) + start3[:, None] - truth3, axis=2).mean(1) * 1e3
    e3 = np.linalg.norm(t3["placed"] - truth3, axis=2).mean(1) * 1e3
    print("three hands: mean vertex error in mm", e0, "->", e3, "pixels", t3["pixels"])
    assert t3["fitted"].tolist() == [True, False, True] and t3["cam_t"][1].tobytes() == start[0].tobytes()
    assert t3["rotation"][1].tobytes() == np.eye(3).tobytes() and t3["pixels"][1] == 0
    assert (t3["counts"][[0, 2], 1] == 0).all() and (t3["counts"][[0, 2], 0, 0] > 100).all()      # direction 2 is switched off for them
    assert e3[0] < e0[0] / 2 and e3[2] < e0[2] / 2
    # steps over the caps are not applied: every hand keeps its bytes
    capped = ME.fit_contour(**one, radius=S["radius"], max_rot_rad=1e-9)
    assert capped["cam_t"].cpu().numpy().tobytes() == start.tobytes() and not bool(capped["fitted"].any())
    render.release_workspaces()
    ME.release_fit_workspaces()


# ------------------------------------------------------------------ g: the drivers, on a synthetic MANO model
class _Cfg:
    ckpt_path = "synthetic:0"
    model_cfg = None
    use_onnx = False
    onnx_path = None


FH, FW = 192, 256
FK = np.array([[300.0, 0.0, 128.0], [0.0, 300.0, 96.0], [0.0, 0.0, 1.0]], np.float32)


def test_refine_to_on_a_synthetic_folder(tmp_path, monkeypatch):
    from PIL import Image
    from hamer_yolo_amd import evaluate_depth as ED
    from hamer_yolo_amd import evaluate_masks as EM
    from hamer_yolo_amd import infer
    hi = infer.hamer_inference(_Cfg)
    monkeypatch.setattr(infer, "hamer_inference", lambda cfg: hi)
    npy_dir, img_dir, mask_dir, out_dir = (tmp_path / d for d in ("npy", "img", "masks", "out"))
    for d in (npy_dir, img_dir, mask_dir):
        d.mkdir()
    np.savetxt(tmp_path / "K.txt", FK)
    rng = np.random.default_rng(21)
    sides = {"b0": ("right",), "b1": ("left",), "b2": ("right", "left"), "b3": ("right",)}
    faces = torch.as_tensor(np.asarray(hi.mano.faces, np.int32), device=DEV)
    for stem, ts in sides.items():
        Image.fromarray(np.zeros((FH, FW, 3), np.uint8)).save(img_dir / f"{stem}.png")
        rec = {"right": None, "left": None}
        for t in ts:
            pg, ph = rng.normal(0, 0.3, 3).astype(np.float32), rng.normal(0, 0.15, 45).astype(np.float32)
            rec[t] = {"betas": rng.normal(0, 0.5, 10).astype(np.float32), "theta": np.concatenate([pg, ph]), "pose_hand": ph,
                      "pose_global": pg, "cam_t": np.array([-0.12 if t == "right" else 0.12, 0.0, 0.7], np.float32), "is_right": t == "right"}
        np.save(npy_dir / f"{stem}.npy", rec)
        # the mask: the hands' own silhouettes at a displaced pose -- 5 % nearer, 10 degrees about the viewing axis, 10 mm aside
        moved = []
        for t in ts:
            pg = ED.fold_rotation(rec[t]["pose_global"], MR.exp_so3(np.array([[0.0, 0.0, np.radians(10.0)]]))[0], t == "right").astype(np.float32)
            cam_t = (rec[t]["cam_t"].astype(np.float64) / 1.05 + np.array([0.008, -0.006, 0.0])).astype(np.float32)
            moved.append(dict(rec[t], pose_global=pg, theta=np.concatenate([pg, rec[t]["pose_hand"]]), cam_t=cam_t))
        verts = render.camera_vertices(hi, moved)
        meshes = [{"frame": 0, "vertices": verts[j], "faces": faces} for j in range(len(moved))]
        mid = render.render_views(FH, FW, FK, meshes, outputs=("mesh_id",), views=1, device=DEV)["mesh_id"][0].cpu().numpy()
        if stem != "b3":                                                               # b3 is given no mask
            np.save(mask_dir / f"{stem}.npy", ((mid >= 0) * 3).astype(np.uint8))
    out_json = tmp_path / "out.json"
    res = EM.main(["--pred", str(npy_dir), "--images", str(img_dir), "--masks", str(mask_dir), "--intrinsics", str(tmp_path / "K.txt"),
                   "--refine-to", str(out_dir), "--fit-radius", "16", "--json", str(out_json)])
    assert res["refine"] == {"records": 4, "hands": 5, "fitted": 4, "skipped": ["b3"], "n_skipped": 1} and ME._fit_ws == {}
    import json
    saved = json.load(open(out_json))
    assert saved["refined"]["frames"].keys() == saved["frames"].keys() == {"b0", "b1", "b2"}
    for stem in ("b0", "b1", "b2"):
        before, after = res["frames"][stem], res["refined"]["frames"][stem]
        print(stem, "J %.4f -> %.4f, F %.4f -> %.4f" % (before["J"], after["J"], before["F"], after["F"]))
        assert after["J"] >= before["J"] and before["J"] < 0.9
    assert res["refined"]["j_mean"] > res["j_mean"] + 0.05
    for stem, ts in sides.items():
        a, b = (np.load(d / f"{stem}.npy", allow_pickle=True).item() for d in (out_dir, npy_dir))
        for t in ("right", "left"):
            assert (a[t] is None) == (t not in ts)
        for t in ts:
            assert set(a[t]) == set(b[t]) | set(EM.FIT_KEYS)
            assert all(TH_same(a[t][k], b[t][k]) for k in b[t] if k not in ("cam_t", "pose_global", "theta"))
            assert TH_same(a[t]["cam_t_unrefined"], b[t]["cam_t"]) and TH_same(a[t]["pose_global_unrefined"], b[t]["pose_global"])
            assert np.array_equal(a[t]["theta"][:3], a[t]["pose_global"]) and np.array_equal(a[t]["theta"][3:], b[t]["theta"][3:])
            if stem == "b3":
                assert all(TH_same(a[t][k], b[t][k]) for k in b[t]) and a[t]["mask_fit"] is False and a[t]["mask_fit_pixels"] == 0
                continue
            assert a[t]["mask_fit"] is True and a[t]["mask_fit_pixels"] >= 30 and np.isfinite(a[t]["mask_fit_rms_px"])
            assert a[t]["cam_t"].dtype == np.float32 and a[t]["pose_global"].dtype == np.float32
    # the record, run through MANO again, is the mesh fit_contour placed
    b0 = np.load(npy_dir / "b0.npy", allow_pickle=True).item()["right"]
    joints, verts = infer.mano_hand_joints_vertices(hi, [b0])
    cam_t = torch.tensor(b0["cam_t"][None], device=DEV)
    r = ME.fit_contour(FH, FW, FK.astype(np.float64)[None], verts, faces, cam_t, joints[:, 0, :].to(torch.float64) + cam_t.to(torch.float64), [0],
                       dev(np.load(mask_dir / "b0.npy")[None]), [3], radius=16)
    got = render.camera_vertices(hi, [np.load(out_dir / "b0.npy", allow_pickle=True).item()["right"]]).cpu().numpy().astype(np.float64)
    worst = np.abs(got[0] - r["placed"][0].cpu().numpy()).max()
    print("record round trip %.2e m" % worst)
    assert worst <= TH.ROUND_TRIP_M
    render.release_workspaces()
    ME.release_fit_workspaces()


def TH_same(a, b):
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    if isinstance(a, float) and np.isnan(a):
        return isinstance(b, float) and np.isnan(b)
    return type(a) is type(b) and a == b


def test_infer_masks_without_mask_fit_writes_the_same_bytes(tmp_path, monkeypatch):
    """On the precise route a hand's bytes do not depend on the run: --masks alone, --mask-fit none and the Python call the
    --masks line has always made write equal files; --mask-fit contour adds the keys."""
    from PIL import Image
    from hamer_yolo_amd import evaluate_masks as EM
    from hamer_yolo_amd import infer, synth
    hi = infer.hamer_inference(_Cfg, precise=True)
    rgb, masks = tmp_path / "rgb", tmp_path / "masks"
    rgb.mkdir(); masks.mkdir()
    for i in range(2):
        Image.fromarray(synth.frame_u8(240, 320, seed=70 + i).numpy()[:, :, ::-1]).save(rgb / f"g{i}.png")
        m = np.zeros((240, 320), np.uint8)
        m[60 + 10 * i:150, 90:170 + 10 * i] = 3
        np.save(masks / f"g{i}.npy", m)
    monkeypatch.setattr(infer, "hamer_inference", lambda cfg: hi)
    outs = [str(tmp_path / d) for d in ("call", "plain", "none", "fit")]
    infer.process_batch_manopara_with_mask(str(rgb), str(masks), outs[0], None, hamer=hi, batched=True, left_label=None, rank=0, world=1,
                                           right_label=3)
    infer.main(["--input", str(rgb), "--output", outs[1], "--masks", str(masks)])
    infer.main(["--input", str(rgb), "--output", outs[2], "--masks", str(masks), "--mask-fit", "none"])
    infer.main(["--input", str(rgb), "--output", outs[3], "--masks", str(masks), "--mask-fit", "contour"])
    for f in ("g0.npy", "g1.npy"):
        raw = [open(os.path.join(o, f), "rb").read() for o in outs]
        assert raw[0] == raw[1] == raw[2]
        a, b = (np.load(os.path.join(o, f), allow_pickle=True).item()["right"] for o in (outs[3], outs[1]))
        assert set(a) == set(b) | set(EM.FIT_KEYS) and TH_same(a["cam_t_unrefined"], b["cam_t"]) and isinstance(a["mask_fit"], bool)
    render.release_workspaces()
