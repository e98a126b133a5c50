"""Mesh overlay and z-buffered renderer measurements (DESIGN.md sections 8 and 8.1).

  python tools/bench_render.py device [--iters 20] [--topology surface|synthetic] [--renderer overlay|zbuffer|both]
                                                     64 synthetic 1080p frames x 4 hands through hm_mesh_overlay (flat; with
                                                     --renderer both: shaded) and / or hm_mesh_render (frames + out, and in a
                                                     second figure rgba + depth + mesh_id); prints the event time per call.
                                                     Run it a second time under
                                                     `rocprofv3 --kernel-trace --stats -- python tools/bench_render.py device`
                                                     for the per-kernel device time (overlay_setup / raster / compose,
                                                     zrender_normals / setup / raster / resolve).
  python tools/bench_render.py device --skeleton [--iters 20]
                                                     64 synthetic 1080p frames x 4 hand skeletons (style 'hamer') through
                                                     hm_skeleton_overlay: the device time (the library's
                                                     own events around its launches, median) of the in-place and of the copying
                                                     form, next to hm_mesh_overlay's compose pass alone (a call without meshes)
                                                     and a device-to-device copy of the same frames, all from this run.
  python tools/bench_render.py folder [--frames 64] [--style flat|shaded|smooth] [--hand-maps]
                                                     render_folder (or hand_maps_folder) on a folder of synthetic 1080p .jpg
                                                     frames with 2 hands each (records made from seeded MANO parameters,
                                                     synthetic:0 weights): frames/s of the whole call (decode, MANO, draw, copy
                                                     back, encode).
Each mode prints one JSON line."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hamer_yolo_amd import render, synth  # noqa: E402

H, W = 1080, 1920


def surface_mesh(nu=26, nv=30, size=0.16):
    """A closed ellipsoid of MANO's size (780 vertices, 1500 faces) whose triangles join neighbouring vertices, as a real hand
    mesh's do.  The synthetic MANO topology (random vertex triples, every face as large as the hand) is the worst case."""
    u = np.linspace(0.05, np.pi - 0.05, nu)[:, None]
    w = np.linspace(0, 2 * np.pi, nv, endpoint=False)[None, :]
    v = np.stack([0.5 * size * np.sin(u) * np.cos(w), 0.5 * size * np.cos(u) + 0 * w, 0.2 * size * np.sin(u) * np.sin(w)], -1)
    idx = np.arange(nu * nv).reshape(nu, nv)
    a, b, c, d = idx[:-1], np.roll(idx, -1, 1)[:-1], idx[1:], np.roll(idx, -1, 1)[1:]
    f = np.concatenate([np.stack([a, b, c], -1).reshape(-1, 3), np.stack([b, d, c], -1).reshape(-1, 3)])
    return v.reshape(-1, 3), f.astype(np.int32)


def _meshes(N, per_frame, seed=0, topology="surface"):
    if topology == "surface":
        v, f = surface_mesh()
        faces = torch.from_numpy(f).cuda()
    else:
        mp = synth.mano_params(seed=0)
        v = mp["v_template"].double().numpy()
        faces = mp["faces"].to(torch.int32).cuda()
    rng = np.random.default_rng(seed)
    out = []
    for n in range(N):
        for k in range(per_frame):
            z = rng.uniform(0.5, 0.9)
            t = np.array([(rng.uniform(0.2, 0.8) * W - W / 2) * z / 1000.0, (rng.uniform(0.2, 0.8) * H - H / 2) * z / 1000.0, z])
            vv = v.copy()
            if k % 2:
                vv[:, 0] = -vv[:, 0]
            out.append({"frame": n, "vertices": torch.from_numpy(vv + t).cuda(), "faces": faces, "is_right": k % 2 == 0})
    return out


def _event_ms(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return round(e0.elapsed_time(e1) / iters, 4)


def device(iters, topology, renderer="overlay"):
    N = 64
    frames = torch.stack([synth.frame_u8(H, W, seed=n) for n in range(N)]).cuda()
    K = np.array([[1000.0, 0, W / 2], [0, 1000.0, H / 2], [0, 0, 1]])
    meshes = _meshes(N, 4, topology=topology)
    out = torch.empty_like(frames)
    frame_bytes = 2 * N * H * W * 3
    res = {"mode": "device", "renderer": renderer, "topology": topology, "frames": N, "hands": len(meshes),
           "faces_per_hand": int(meshes[0]["faces"].shape[0]), "frame_bytes_read_written": frame_bytes,
           "hbm_floor_ms_at_8TBps": round(frame_bytes / 8e12 * 1e3, 4)}
    if renderer == "overlay":
        res["ms_per_call_events_incl_host_prep"] = _event_ms(lambda: render.overlay_frames(frames, K, meshes, out=out), iters)
    if renderer == "both":
        res["overlay_shaded_ms_per_call"] = _event_ms(lambda: render.overlay_frames(frames, K, meshes, style="shaded", out=out), iters)
    if renderer in ("zbuffer", "both"):
        res["zbuffer_frames_out_ms_per_call"] = _event_ms(lambda: render.render_views(H, W, K, meshes, frames=frames, outputs=()), iters)
        res["zbuffer_rgba_depth_id_ms_per_call"] = _event_ms(lambda: render.render_views(H, W, K, meshes, views=N), iters)
    print(json.dumps(res))


def _library_ms(fn, iters):
    """Median device time of the library call(s) inside fn: the events the library records around its own launches."""
    from hamer_yolo_amd import lib as L
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    with L.profile() as p:
        for _ in range(iters):
            fn()
    return round(float(np.median([r[5] for r in p.records])), 4)


def skeleton(iters):
    N, per_frame = 64, 4
    frames = torch.stack([synth.frame_u8(H, W, seed=n) for n in range(N)]).cuda()
    rng = np.random.default_rng(0)
    kp = np.empty((N * per_frame, 21, 2), np.float32)
    for i in range(N * per_frame):                              # a hand about 250 px across, anywhere in the frame
        cx, cy = rng.uniform(0.1, 0.9) * W, rng.uniform(0.1, 0.9) * H
        kp[i] = rng.uniform([cx - 125, cy - 125], [cx + 125, cy + 125], (21, 2))
    kpd = torch.from_numpy(kp).cuda()
    index = [i // per_frame for i in range(N * per_frame)]
    out, work = torch.empty_like(frames), frames.clone()
    K = np.array([[1000.0, 0, W / 2], [0, 1000.0, H / 2], [0, 0, 1]])
    res = {"mode": "device", "what": "skeleton", "style": "hamer", "frames": N, "hands": len(index),
           "frame_bytes": N * H * W * 3, "iters": iters,
           "skeleton_in_place_ms": _library_ms(lambda: render.skeleton_frames(work, kpd, index, inplace=True), iters),
           "skeleton_copying_ms": _library_ms(lambda: render.skeleton_frames(frames, kpd, index, out=out), iters),
           "mesh_overlay_compose_only_ms": _library_ms(lambda: render.overlay_frames(frames, K, [], out=out), iters)}
    times = []
    for _ in range(iters + 3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); out.copy_(frames); e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    res["device_to_device_copy_ms"] = round(float(np.median(times[3:])), 4)
    touched = (work != frames).any(-1).sum().item()
    res["pixels_drawn_fraction"] = round(touched / (N * H * W), 5)
    print(json.dumps(res))


class _Cfg:
    ckpt_path = "synthetic:0"
    model_cfg = None
    use_onnx = False
    onnx_path = None


def folder(n_frames, style="flat", hand_maps=False):
    from PIL import Image
    from hamer_yolo_amd.infer import hamer_inference
    hi = hamer_inference(_Cfg)
    rng = np.random.default_rng(0)
    with tempfile.TemporaryDirectory() as d:
        img, npy, out = (os.path.join(d, s) for s in ("rgb", "npy", "out"))
        os.makedirs(img); os.makedirs(npy)
        for i in range(n_frames):
            Image.fromarray(synth.frame_u8(H, W, seed=i).numpy()[:, :, ::-1]).save(os.path.join(img, f"{i:06d}.jpg"), quality=90)
            rec = {}
            for t, x in (("right", -0.08), ("left", 0.08)):
                pg, ph = rng.normal(0, 0.3, 3).astype(np.float32), rng.normal(0, 0.2, 45).astype(np.float32)
                rec[t] = {"betas": rng.normal(0, 0.5, 10).astype(np.float32), "theta": np.concatenate([pg, ph]), "pose_hand": ph,
                          "pose_global": pg, "cam_t": np.array([x, 0.02, 0.6], np.float32), "is_right": t == "right"}
            np.save(os.path.join(npy, f"{i:06d}.npy"), rec)
        if hand_maps:
            run = lambda **kw: render.hand_maps_folder(img, npy, out, hi, **kw)
        else:
            run = lambda **kw: render.render_folder(img, npy, out, hi, style=style, **kw)
        run(frames_per_pass=8)                                                  # warm-up: code objects, workspace
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n = run()
        dt = time.perf_counter() - t0
    print(json.dumps({"mode": "folder", "what": "hand_maps" if hand_maps else style, "frames": n, "seconds": round(dt, 3),
                      "frames_per_s": round(n / dt, 2), "threads": render._encode_threads()}))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["device", "folder"])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--topology", choices=["surface", "synthetic"], default="surface")
    ap.add_argument("--renderer", choices=["overlay", "zbuffer", "both"], default="overlay")
    ap.add_argument("--style", choices=["flat", "shaded", "smooth"], default="flat")
    ap.add_argument("--hand-maps", action="store_true")
    ap.add_argument("--skeleton", action="store_true", help="device mode: measure hm_skeleton_overlay instead of the mesh renderers")
    a = ap.parse_args()
    if a.mode == "device" and a.skeleton:
        skeleton(a.iters)
    else:
        device(a.iters, a.topology, a.renderer) if a.mode == "device" else folder(a.frames, a.style, a.hand_maps)
