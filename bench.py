#!/usr/bin/env python3
"""bench.py -- hands/sec of the HaMeR hot path on MI355X (BASELINE.json configs[1]).

A step = one forward of hm_hamer_forward (patch gather, ViT-H/16 backbone, transformer-decoder
MANO head, rot6d + MANO LBS + projection) over one batch of 64 synthetic 256x256 crops that are
already resident in HBM, 16-bit MFMA GEMMs (fp16 operands: the type that meets the 1e-3 parity bar
on fp32 master weights; --dtype bf16 selects the other), detector bypassed.  With N > 1 (launched by
torch.distributed.run, one rank per GPU) every rank processes its own 64-crop shard (weak
scaling); RCCL carries the one-off weight broadcast and the per-step gather of per-hand MANO
parameters to rank 0.

Prints ONE JSON line on rank 0 (see the field list in DESIGN.md section "Measurement").  A plain run sets up, warms up, times
--steps steps and prints the line; --full adds what the headline does not need (the event-timed roofline pass, the side
configurations, the CPU baselines).  --dump-outputs DIR writes the last timed step's outputs for output-for-output comparisons.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from hamer_yolo_amd import lib as L  # noqa: E402
from hamer_yolo_amd import shard, synth  # noqa: E402
from hamer_yolo_amd.engine import HamerEngine  # noqa: E402

PEAK_BF16_TFLOPS = 2500.0   # dense bf16/fp16 MFMA peak, /opt/skills/guides/MI355X_MICROARCH.md
EPI_NAMES = {0: "store", 1: "gelu", 2: "resid_f32", 3: "f32", 4: "silu", 5: "resid_ln", 6: "ln_store", 7: "ln_gelu",
             16: "fp8_store", 18: "fp8_resid_f32", 24: "fp8_gelu_mx8"}
PEAK_FP8_TFLOPS = 5000.0       # dense e4m3 on the block-scaled 16x16x128 MFMA (MI355X_MICROARCH.md)


def flops_per_hand(cfg: synth.HamerConfig) -> dict:
    v, d = cfg.vit, cfg.dec
    T, D, H = v.tokens, v.embed_dim, v.embed_dim * v.mlp_ratio
    blk = 2 * T * D * 3 * D + 2 * 2 * T * T * D + 2 * T * D * D + 2 * 2 * T * D * H
    patch = 2 * T * 3 * v.patch * v.patch * D
    kv = 2 * T * d.context_dim * d.depth * 2 * d.inner
    return {"vit": patch + v.depth * blk, "decoder_kv": kv, "total_mfma": patch + v.depth * blk + kv}


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(out_dir: str, arrays: dict) -> None:
    """--dump-outputs: what the timed path returned in its last step, one out_dir/<name>.npy per array (float64 stays
    float64, everything else becomes float32), so that two builds can be compared output for output on the same seeded
    inputs.  Every array has one row per hand; above DUMP_LIMIT_BYTES in all, the same seeded sample of rows is kept of each."""
    arrays = {k: (v.detach().float().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in arrays.items()}
    arrays = {k: v if v.dtype == np.float64 else v.astype(np.float32) for k, v in arrays.items()}
    total = sum(v.nbytes for v in arrays.values())
    if total > DUMP_LIMIT_BYTES:
        n = len(next(iter(arrays.values())))
        keep = np.sort(np.random.default_rng(0).choice(n, max(1, n * DUMP_LIMIT_BYTES // (total + 8 * n)), replace=False))
        arrays = {k: v[keep] for k, v in arrays.items()}
        arrays["sampled_rows"] = keep.astype(np.float64)
    os.makedirs(out_dir, exist_ok=True)
    for k, v in arrays.items():
        np.save(os.path.join(out_dir, k + ".npy"), v)


def host_threads() -> int:
    """Host cores this process may really use: HAMER_CPU_THREADS, else the cgroup CPU quota,
    else min(affinity, 16) (a one-GPU box's share of the host is 16 cores)."""
    if os.environ.get("HAMER_CPU_THREADS"):
        return max(1, int(os.environ["HAMER_CPU_THREADS"]))
    n = len(os.sched_getaffinity(0))
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period))))
    except (OSError, ValueError):
        pass
    return max(1, min(n, 16))


def cpu_baseline(cfg, sd_dev, mano_cpu, seconds: float = 12.0):
    """The oracle (CPU restatement of the reference path, fp32 PyTorch, fp32 weights) timed on the host cores: the reference's
    own mode of operation B = 1 (configs[0]: one crop per forward, infer.py:1268-1274) and B = 8."""
    from oracle import hamer_ref as R
    threads = host_threads()
    torch.set_num_threads(threads)
    sd = {k: v.float().cpu() for k, v in sd_dev.items()}
    res = {}
    with torch.no_grad():
        R.hamer_forward(sd, mano_cpu, synth.normalize_crops(synth.crops_u8(1, seed0=0)), cfg)      # warm-up
        for B, budget, cap in ((1, seconds * 0.4, 12), (8, seconds, 6)):
            img = synth.normalize_crops(synth.crops_u8(B, seed0=0))
            n, t0 = 0, time.perf_counter()
            while True:
                R.hamer_forward(sd, mano_cpu, img, cfg)
                n += 1
                dt = time.perf_counter() - t0
                if dt >= budget or n >= cap:
                    break
            res[B] = (n, dt)
    n8, dt8 = res[8]
    n1, dt1 = res[1]
    return {"value": round(n8 * 8 / dt8, 3), "unit": "hands/s", "cores": threads, "kind": "port",
            "value_b1": round(n1 / dt1, 3), "s_per_hand_b1": round(dt1 / n1, 4),
            "sample": f"{n8} forwards of B=8 crops ({dt8:.1f} s) and {n1} forwards of B=1 ({dt1:.1f} s; configs[0]: the reference "
                      f"processes one crop per forward), ViT-H/16 + decoder + MANO, fp32 torch CPU oracle"}


def cpu_baseline_detector(yolo_weights: str, seconds: float = 8.0):
    """the detector leg of configs[2] on the host cores -- the oracle restatement of Detector.detect
    (yolo/detector.py:106-153: letterbox, fused YOLOv7 forward in fp32 as the reference's CPU branch :110-112, decode, NMS,
    scale_coords) on ONE seeded 1080p frame, repeated for a bounded time."""
    from hamer_yolo_amd.yolo import arch, fuse
    from hamer_yolo_amd.yolo.detector import attempt_load
    from oracle import yolo_ref
    threads = host_threads()
    torch.set_num_threads(threads)
    sd, nc, _ = attempt_load(yolo_weights)
    layers = arch.yolov7_layers()
    fused = fuse.fuse_state_dict(sd, arch.conv_specs(layers, 3, nc))
    frame = synth.frame_u8(1080, 1920, seed=0).numpy()
    with torch.no_grad():
        yolo_ref.detect(layers, fused, frame, nc, arch.ANCHORS)                 # warm-up
        n, t0 = 0, time.perf_counter()
        while True:
            dets = yolo_ref.detect(layers, fused, frame, nc, arch.ANCHORS)[0]
            n += 1
            dt = time.perf_counter() - t0
            if dt >= seconds or n >= 200:
                break
    return {"value": round(n / dt, 3), "unit": "frames/s", "s_per_frame": round(dt / n, 4), "cores": threads, "kind": "port",
            "sample": f"{n} passes of one seeded 1080p frame ({dt:.1f} s): letterbox + fused YOLOv7 fp32 + decode + NMS + scale_coords, "
                      f"torch CPU oracle (oracle/yolo_ref.detect), {len(dets)} boxes"}


def run_e2e(args, dev, dtype, yolo_weights="synthetic:2:-2.2:0", chunks_per_pass: int = 4, long_chunks: int = 0, rank: int = 0,
            world: int = 1, want_roofline: bool = False):
    """BASELINE configs[2], timed through the product driver itself: a folder of seeded 1080p frames on disk ->
    hamer_yolo_amd.infer.process_batch_manopara (thread-pool decode into page-locked slots, detector passes of --frames frames at
    the start and up to 48 afterwards: one batched YOLOv7 pass + NMS each, hands queued across frames and cropped 64 at a time
    into ONE HaMeR forward, camera step, batches in flight on two streams) -> one .npy per frame.  A step = one pass over the
    folder, value = hands that went through HaMeR per second (file decode and .npy writes included).
    With N ranks (torch.distributed.run) the folder holds N x as many frames and rank r takes files r, r + N, ... on its own GPU
    (weak scaling; no data-path collective, one all_reduce of the counts after the timed region)."""
    import glob
    import shutil
    import tempfile
    import numpy as np
    import torch.distributed as dist
    from hamer_yolo_amd import infer
    from hamer_yolo_amd.yolo.detector import Detector

    class YCfg:
        weights = yolo_weights; imgsz = 640; augment = True; conf_thres = 0.25; iou_thres = 0.35
        classes = [0, 1, 2]; agnostic_nms = True; device = str(dev); save_path = "./output"

    class HCfg:
        ckpt_path = "synthetic:0"; model_cfg = None; use_onnx = False; onnx_path = None

    from PIL import Image
    F = args.frames
    multi = world > 1
    root_box = [tempfile.mkdtemp(prefix="hamer_e2e_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None) if rank == 0 else None]
    if multi:
        dist.broadcast_object_list(root_box, src=0)
    root = root_box[0]
    try:
        in_dir = os.path.join(root, "rgb")
        per_rank = F * chunks_per_pass             # frames per rank and pass; fill and drain of the pipeline are part of a pass
        n_frames = per_rank * world

        def link_frames(lo, hi):
            for i in range(lo, hi):                # the eight seeded frames repeat: hard links, every file is still read and decoded
                os.link(os.path.join(in_dir, f"f{i % 8:05d}.bmp"), os.path.join(in_dir, f"f{i:05d}.bmp"))

        if rank == 0:
            os.makedirs(in_dir)
            for i in range(8):                     # uncompressed .bmp: the decode is a copy, not an inflate
                Image.fromarray(synth.frame_u8(1080, 1920, seed=i).numpy()[:, :, ::-1]).save(os.path.join(in_dir, f"f{i:05d}.bmp"))
            link_frames(8, n_frames)
        if multi:
            dist.barrier()
        hi = infer.hamer_inference(HCfg)
        det = Detector(YCfg)
        sar, k_real = None, None
        if args.workload == "e2e-depth":                   # d_infer.py: + RootNet root depth per hand
            from hamer_yolo_amd import d_infer
            from hamer_yolo_amd.rootnet.Model_RGB import get_model
            sar = get_model()                              # synthetic ResNet-34 + depth head (rootnet/sar_config_stage_1.py)
            k_real = np.array([[1400.0, 0, 960], [0, 1400.0, 540], [0, 0, 1]], np.float32)
        n_out = [0]

        def step(**kw):
            out_dir = os.path.join(root, f"out_r{rank}_{n_out[0]}")      # (a fresh folder per pass: no deletes inside the timed region)
            n_out[0] += 1
            if getattr(args, "det_frames", 0):
                kw.setdefault("det_frames", args.det_frames)
            if sar is not None:
                return d_infer.process_batch_manopara(in_dir, out_dir, k_real, hamer=hi, detector=det, sar=sar, frames_per_step=F,
                                                      rank=rank, world=world, **kw), out_dir
            return infer.process_batch_manopara(in_dir, out_dir, None, hamer=hi, detector=det, frames_per_step=F,
                                                rank=rank, world=world, **kw), out_dir

        def timed(n_steps):
            torch.cuda.synchronize()
            if multi:
                dist.barrier()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            hands = 0
            for _ in range(n_steps):
                st, od = step()
                hands += st["hands"]
            torch.cuda.synchronize()
            if multi:
                dist.barrier()
            torch.cuda.synchronize()
            el = time.perf_counter() - t0
            if multi:
                t = torch.tensor([el, float(hands)], device=dev, dtype=torch.float64)
                dist.all_reduce(t[:1], op=dist.ReduceOp.MAX)
                dist.all_reduce(t[1:], op=dist.ReduceOp.SUM)
                el, hands = float(t[0].item()), int(round(float(t[1].item())))
            return el, hands, st, od

        import contextlib, io
        with contextlib.redirect_stdout(io.StringIO()):
            for _ in range(max(1, args.warmup)):
                step()
            el, hands_all, st, od = timed(args.steps)
        hands = hands_all // args.steps                        # hands FORWARDED per pass, all ranks (boxes without area never get there)
        files = sorted(glob.glob(os.path.join(od, "*.npy")))
        if getattr(args, "dump_outputs", None) and rank == 0:
            # the hands of the last timed pass in file order, left before right: one row per hand in every array
            rows = [(int(os.path.basename(f)[1:-4]), float(side == "right"), r) for f in files
                    for side, r in sorted(np.load(f, allow_pickle=True).item().items()) if r is not None]
            dump_outputs(args.dump_outputs, {"frame": np.array([n for n, _, _ in rows], np.float64),
                                             "is_right": np.array([s for _, s, _ in rows], np.float64),
                                             **{k: np.stack([r[k] for _, _, r in rows]) if rows else np.zeros((0,))
                                                for k in ("betas", "theta", "cam_t")}})
        files = len(files)
        roof = None
        if want_roofline and not multi:
            # the two MFMA kernel families of this workload, each launch timed alone: one pass of the same driver with the
            # detector on the HaMeR stream and one batch in flight (hipEvent pairs around every launch, hm_prof_*)
            with contextlib.redirect_stdout(io.StringIO()), L.profile(capacity=1 << 16) as prof:
                step(in_flight=1, overlap_detector=False)
                torch.cuda.synchronize()
            fam = {"gemm": [0.0, 0.0, 0], "conv": [0.0, 0.0, 0]}
            other = {}
            for kind, epi, M, N, K, ms in prof.records:
                if kind in fam:
                    fam[kind][0] += 2.0 * M * N * K; fam[kind][1] += ms; fam[kind][2] += 1
                else:
                    other[kind] = other.get(kind, 0.0) + ms
            roof = {k: {"achieved": round(v[0] / (v[1] * 1e-3) / 1e12, 2), "peak": PEAK_BF16_TFLOPS, "unit": "TFLOP/s",
                        "frac": round(v[0] / (v[1] * 1e-3) / 1e12 / PEAK_BF16_TFLOPS, 4), "launches_per_pass": v[2],
                        "ms_per_pass": round(v[1], 3), "gflop_per_pass": round(v[0] / 1e9, 1)} for k, v in fam.items() if v[1] > 0}
            roof["bound"] = "mfma"
            roof["other_ms_per_pass"] = {k: round(v, 3) for k, v in sorted(other.items(), key=lambda kv: -kv[1])}
            roof["timing"] = "hipEvent pairs around every launch; one serial pass of the same driver (detector on the HaMeR stream, one batch in flight)"
        long_pass = None
        if long_chunks > chunks_per_pass and not multi:    # the same models over a longer folder (same eight frames, more links)
            n_long = F * long_chunks
            link_frames(n_frames, n_long)
            with contextlib.redirect_stdout(io.StringIO()):
                step()
                el2, hands2, _, _ = timed(2)
            long_pass = {"value": round(hands2 / el2, 2), "ms_per_step": round(1e3 * el2 / 2, 3), "frames_per_pass": n_long,
                         "frames_per_s": round(2 * n_long / el2, 2), "hands_per_pass": hands2 // 2}
        if multi:
            dist.barrier()
    finally:
        if rank == 0:
            shutil.rmtree(root, ignore_errors=True)
    return           ({"metric": "hands/sec end-to-end (files -> YOLOv7 -> " + ("RootNet depth + " if sar is not None else "") + "crop -> HaMeR -> MANO -> .npy), 1080p frames",
                      "value": round(hands_all / el, 2), "unit": "hands/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
                      "ms_per_step": round(1e3 * el / args.steps, 3), "frames_per_pass": n_frames, "hands_per_pass": hands,
                      "hands_per_frame": round(hands / n_frames, 2), "frames_per_s": round(n_frames * args.steps / el, 2),
                      "npy_files_per_pass_rank0": files, "higher_is_better": True, "scaling": "weak",
                      "dtype": args.dtype + " (HaMeR) / fp16 (YOLOv7)", "data": "synthetic",
                      "config": {"workload": ("d_infer.py flow: 1080p frames through YOLOv7 + RootNet (ResNet-34 root depth per hand) + HaMeR via "
                                              "d_infer.process_batch_manopara, detector boxes used as found") if sar is not None else
                                             ("BASELINE configs[2]: 1080p frames through yolo/detector.py YOLOv7 + HaMeR via "
                                              "infer.process_batch_manopara (the README entry point), detector boxes used as found"),
                                 "first_detector_pass_frames": F, "detector_pass_frames": getattr(args, "det_frames", 0) or infer.DET_FRAMES, "hands_per_forward": infer.HANDS_PER_FORWARD,
                                 "batches_in_flight": 2, "detector_weights": yolo_weights, "frames_per_rank_and_pass": per_rank,
                                 "parallelism": f"frames round-robin x{world}", "forwards_per_pass_rank0": st.get("forwards"), "forward_sizes_rank0": st.get("forward_sizes"), "detector_pass_sizes_rank0": st.get("det_pass_sizes"),
                                 "detector_passes_per_pass_rank0": st.get("det_passes")},
                      "gflop_per_frame": round(61.9 + hands / n_frames * 251.03, 1),
                      **({"roofline": roof} if roof else {}), **({"long_pass": long_pass} if long_pass else {})})


E2E_WEIGHTS_4_HANDS = "synthetic:2:-2.53:0"     # objectness bias calibrated on the 8 seeded frames to ~4 boxes per frame (tools/probes/yolo_hands_per_frame.py)


def side_configs(args, dev, cfg, sd, mano_cpu, eng, contract_value, ctxs):
    """The other single-GPU BASELINE configurations, timed briefly in the same process so that the driver's one command observes
    them too; --full only.  Not the contract line: `value` above stays configs[1].  ~40 s in all."""
    import types
    out = {}
    t_all = time.perf_counter()
    only = os.environ.get("HAMER_BENCH_SIDE", "shard,fp8,e2e").split(",")     # (debugging: a subset of the side configurations)

    def side_shard():
        # configs[3] at N = 1: the shard job (1024 crops, forwards of 64 on two contexts, pack + gather) -- shard.ShardJob
        mine = synth.normalize_crops(synth.crops_u8(1024, seed0=0)).to(dev)
        job = shard.ShardJob(eng, mine, 1024, batch=64, in_flight=2, contexts=ctxs)    # the contract line's own streams and workspaces
        job.step(); job.step(); torch.cuda.synchronize()      # (two warm-up jobs: the profiling pass before this left the chip idle)
        NJ = 3
        t0 = time.perf_counter()
        for _ in range(NJ):
            last = job.step()
        torch.cuda.synchronize()
        el = time.perf_counter() - t0
        assert last.shape == (1024, shard.PARAMS_PER_HAND) and bool(torch.isfinite(last).all())
        return {"value": round(NJ * 1024 / el, 1), "unit": "hands/s", "ms_per_job": round(el / NJ * 1e3, 2), "jobs": NJ,
                "vs_contract_line": round(NJ * 1024 / el / contract_value, 4), "dtype": "fp16"}

    def side_fp8():
        # configs[4]: fp8 ViT-H, B = 256, two batches in flight
        e8 = HamerEngine(sd, mano_cpu, cfg, device=dev, fp8=True)
        c8 = e8.contexts(256, 2)
        img8 = synth.normalize_crops(synth.crops_u8(256, seed0=0)).to(dev)

        def step8(i):
            c = c8[i % 2]
            with torch.cuda.stream(c.stream):
                e8.forward(img8, c.out, workspace=c.workspace)
        for i in range(4):
            step8(i)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(8):
            step8(i)
        torch.cuda.synchronize()
        el = time.perf_counter() - t0
        assert all(bool(torch.isfinite(c.out["pred_vertices"]).all()) for c in c8)
        fl = flops_per_hand(cfg)["total_mfma"]
        # roofline of this configuration's dominant kernels (the fp8 GEMMs), each launch timed alone: two serial forwards
        with L.profile(capacity=2 * 512) as prof:
            for _ in range(2):
                e8.forward(img8, c8[0].out, workspace=c8[0].workspace)
            torch.cuda.synchronize()
        per, other = {}, {}
        for kind, epi, M_, N_, K_, ms in prof.records:
            if kind == "gemm" and epi >= 16:
                e = per.setdefault(EPI_NAMES[epi], [0, 0.0, 0.0])
                e[0] += 1; e[1] += ms; e[2] += 2.0 * M_ * N_ * K_
            else:
                other[kind] = other.get(kind, 0.0) + ms
        f8_fl, f8_ms = sum(v[2] for v in per.values()), sum(v[1] for v in per.values())
        ach = f8_fl / (f8_ms * 1e-3) / 1e12
        roof = {"kernel": "gemm_fp8p_kernel (store / gelu_mx8) + gemm_fp8_kernel (resid_f32)", "bound": "mfma", "achieved": round(ach, 2),
                "peak": PEAK_FP8_TFLOPS, "unit": "TFLOP/s", "frac": round(ach / PEAK_FP8_TFLOPS, 4),
                "per_epilogue": {k: {"launches_per_step": v[0] // 2, "avg_ms": round(v[1] / v[0], 5), "tflops": round(v[2] / (v[1] * 1e-3) / 1e12, 2)} for k, v in per.items()},
                "other_ms_per_step": {k: round(v / 2, 3) for k, v in sorted(other.items(), key=lambda kv: -kv[1])},
                "traffic": "profiles/r04_pmc_fp8_b256.json (rocprofv3 --pmc over this configuration: bytes beyond L2 and MFMA busy per kernel)",
                "timing": "hipEvent pairs around every launch, two serial forwards after the timed region"}
        return {"value": round(8 * 256 / el, 1), "unit": "hands/s", "ms_per_step": round(el / 8 * 1e3, 2), "steps": 8,
                "dtype": "fp8 (e4m3 weights, MXFP8 activations) / bf16 / fp32",
                "model_frac_of_fp8_peak": round(8 * 256 / el * fl / 1e12 / PEAK_FP8_TFLOPS, 4), "roofline": roof,
                "parity_note": "vertices 3.5e-3 from the fp32 reference (DESIGN.md): not the 1e-3 configuration"}

    def side_e2e():
        # configs[2]: 1080p frames through the product driver, detector calibrated to ~4 hands per frame
        a2 = types.SimpleNamespace(frames=16, steps=3, warmup=1, workload="e2e", dtype="fp16")
        r = run_e2e(a2, dev, torch.float16, yolo_weights=E2E_WEIGHTS_4_HANDS, chunks_per_pass=4, long_chunks=12, want_roofline=True)
        o = {k: r[k] for k in ("value", "unit", "ms_per_step", "frames_per_pass", "hands_per_pass", "hands_per_frame", "frames_per_s",
                               "npy_files_per_pass_rank0", "dtype", "gflop_per_frame", "roofline")}
        o["vs_contract_line"] = round(r["value"] / contract_value, 4)
        o["detector_weights"] = E2E_WEIGHTS_4_HANDS
        o["pipeline"] = {k: r["config"][k] for k in ("first_detector_pass_frames", "detector_pass_frames", "hands_per_forward",
                                                     "forwards_per_pass_rank0", "detector_passes_per_pass_rank0", "forward_sizes_rank0", "detector_pass_sizes_rank0")}
        # long_pass: the same driver and models over a folder three times as long -- a 64-frame pass cannot hide the fill of
        # the pipeline (decode + upload + detector pass of the first frames with nothing to overlap) and its drain
        o["long_pass"] = r["long_pass"]
        o["long_pass"]["vs_contract_line"] = round(r["long_pass"]["value"] / contract_value, 4)
        if not args.no_cpu_baseline:
            o["cpu_baseline_detector"] = cpu_baseline_detector(E2E_WEIGHTS_4_HANDS)
        return o

    # (e2e first: behind the other two its 64-frame pass read 96.8 ms against 92.4 on its own, same box -- profiles/r04_bench_v9_*)
    for key, name, fn in (("e2e", "configs[2] e2e 1080p, ~4 hands/frame", side_e2e), ("shard", "configs[3] shard1024, N=1", side_shard),
                          ("fp8", "configs[4] fp8 ViT-H, B=256", side_fp8)):
        if key in only:
            out[name] = fn()
            torch.cuda.empty_cache()
    out["seconds"] = round(time.perf_counter() - t_all, 1)
    return out


def tome_tokens(eng):
    t, out = eng.tokens, []
    for r in eng.tome_r:
        t -= min(r, t // 2)
        out.append(t)
    return out


def latest_profile(suffix: str):
    """profiles/rNN_<suffix> of the newest round that has one (the PMC passes are collected per round, tools/collect_profiles.sh)."""
    import glob
    found = sorted(glob.glob(os.path.join(ROOT, "profiles", "r[0-9][0-9]_" + suffix)))
    return found[-1] if found else None


def mfma_busy_pmc(cfg):
    """MFMA-pipe busy fraction of the GEMM launches of one step from the committed PMC pass (rocprofv3 --pmc
    SQ_VALU_MFMA_BUSY_CYCLES GRBM_GUI_ACTIVE over tools/pmc_shapes.py; profiles/r01_pmc_mfma_busy.json), cycle-weighted."""
    path = latest_profile("pmc_mfma_busy.json")
    if path is None:
        return None
    t = json.load(open(path))
    w = {"patch": 1, "qkv": cfg.vit.depth, "proj": cfg.vit.depth, "fc1": cfg.vit.depth, "fc2": cfg.vit.depth, "kv": 1}
    busy = sum(t[k]["SQ_VALU_MFMA_BUSY_CYCLES"] * n for k, n in w.items())
    cyc = sum(t[k]["shader_cycles"] * 1024 * n for k, n in w.items())      # (1024 SIMDs)
    return round(busy / cyc, 4)


def relaunch_under_torchrun(n: int) -> int:
    """`bench.py --gpus N` started as a plain process: start N ranks as CHILD processes through torch.distributed.run --
    before this process has touched the GPU (it never does) -- and return their exit code."""
    import socket
    import subprocess
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.call(cmd, env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0")))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=64, help="crops per GPU per forward (BASELINE config: 64)")
    ap.add_argument("--dtype", default="fp16", choices=["fp16", "bf16", "fp8"],
                    help="GEMM operand type.  fp16 (default) meets the 1e-3 parity bar on fp32 master weights, bf16 does not "
                         "(DESIGN.md section 2); fp8: BASELINE configs[4] (qkv/proj/fc1/fc2 on the fp8 MFMA), use with --batch 256")
    ap.add_argument("--workload", default="crops", choices=["crops", "shard1024", "e2e", "e2e-depth"],
                    help="crops: BASELINE configs[1] (default, the contract line; weak scaling: --batch crops per GPU per step); "
                         "shard1024: configs[3], 1024 crops in all, ceil(1024/N) per GPU in forwards of --batch, MANO parameters "
                         "gathered to rank 0 (strong scaling; a step = the whole 1024-crop job); e2e: configs[2], 1080p frames on "
                         "disk through the product driver infer.process_batch_manopara")
    ap.add_argument("--crops", type=int, default=1024, help="shard1024: crops in the whole job")
    ap.add_argument("--frames", type=int, default=16, help="e2e: frames of the first detector pass (later passes take up to 48; HaMeR forwards are 64 hands)")
    ap.add_argument("--in-flight", type=int, default=0,
                    help="batches in flight: consecutive forwards alternate between this many HIP streams (own workspace and outputs "
                         "each), so one batch's HBM-bound phases overlap another's MFMA phases; 1 = strictly one after the other; "
                         "default 2")
    ap.add_argument("--token-merge", action="store_true",
                    help="HAMER_INFER(token_merge=True): ToMe with the reference's schedule r = (8, -1) (SURVEY 8f rank 4); not the contract line")
    ap.add_argument("--fold-ln", action="store_true", help="deferred LayerNorm (LN1/LN2 folded into the neighbouring GEMM epilogues)")
    ap.add_argument("--gemm-variant", type=int, default=-1, help="force one GEMM tile variant (tuning runs)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-side", action="store_true", help="skip the short runs of the other single-GPU BASELINE configurations ('side_configs')")
    ap.add_argument("--chunks", type=int, default=4, help="e2e: a pass (= a step) covers frames x chunks files per GPU")
    ap.add_argument("--det-frames", type=int, default=0, help="e2e: frames per detector pass after the first (default: infer.DET_FRAMES)")
    ap.add_argument("--hands4", action="store_true", help="e2e: detector weights calibrated to ~4 hands per frame (configs[2]'s wording) instead of ~8.6")
    ap.add_argument("--no-roofline", action="store_true")
    ap.add_argument("--full", action="store_true",
                    help="after the headline line's own steps, also what it does not need: the event-timed roofline pass, the side "
                         "configurations (default line only) and the CPU baselines; --no-roofline / --no-side / --no-cpu-baseline "
                         "leave parts of it out")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the timed path computed in its last step as DIR/<name>.npy "
                         "(float32, rank 0's share; at most 64 MB in all)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        raise SystemExit(relaunch_under_torchrun(args.gpus))         # children do the work; nothing here has initialised HIP
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: the hot path has no CPU fallback")
    # HAMER_BENCH_REHEARSAL=1 (one-GPU box): the N > 1 code path with every rank on the one card and gloo as the backend (RCCL
    # refuses two ranks on one device) -- a correctness rehearsal of the rank logic, never a measurement
    rehearsal = os.environ.get("HAMER_BENCH_REHEARSAL") == "1"
    if rehearsal:
        local0 = int(os.environ.get("LOCAL_RANK", "0")) % max(1, torch.cuda.device_count())
        torch.cuda.set_device(local0)
    rank, local, world = shard.init_distributed("gloo" if rehearsal else "nccl")
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    if rehearsal:
        local = local % max(1, torch.cuda.device_count())
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    dist = torch.distributed
    cfg = synth.HamerConfig()
    dtype = torch.float16 if args.dtype == "fp16" else torch.bfloat16
    B = args.batch

    if args.workload in ("e2e", "e2e-depth"):
        res = run_e2e(args, dev, dtype, yolo_weights=E2E_WEIGHTS_4_HANDS if args.hands4 else "synthetic:2:-2.2:0",
                      chunks_per_pass=args.chunks, rank=rank, world=world, want_roofline=args.full and not args.no_roofline)
        if world > 1:
            dist.barrier()
            dist.destroy_process_group()
        if rank == 0:
            print(json.dumps(res), flush=True)
        return

    # weights: rank 0 draws the synthetic checkpoint (fp32 master weights), RCCL broadcasts it as two flat buffers
    sd0 = synth.hamer_state_dict(cfg, seed=0, device=dev) if rank == 0 else None
    # (fp8: the matrices that become e4m3 travel as fp32 -- quantising a copy already rounded to 16 bits would round twice and
    # make the e4m3 bytes and scales depend on the world size)
    sd = shard.broadcast_state_dict(sd0, dev, src=0, half_dtype=torch.float32 if args.dtype == "fp8" else dtype) if shard._multi() else sd0
    mano_cpu = synth.mano_params(seed=0)
    eng = HamerEngine(sd, mano_cpu, cfg, device=dev, dtype=dtype, fp8=(args.dtype == "fp8"), fold_ln=args.fold_ln or None,
                      token_merge=True if args.token_merge else None)
    if args.gemm_variant >= 0:
        L.check(L.load().hm_gemm_set_variant(args.gemm_variant), "hm_gemm_set_variant")
    nfl = args.in_flight if args.in_flight > 0 else 2
    out = eng.alloc_outputs(B)
    eng.workspace(B)

    if args.workload == "shard1024":
        # configs[3]: this rank's contiguous share of the seeded crop set, resident in HBM, in forwards of B crops
        lo, hi = shard.shard_range(args.crops, rank, world)
        mine = synth.normalize_crops(synth.crops_u8(hi - lo, seed0=lo)).to(dev) if hi > lo else None
        job = shard.ShardJob(eng, mine, args.crops, batch=B, in_flight=nfl)       # the step tests/test_gpu_shard.py checks
        ctxs = job.ctxs
        step = job.step
        units_per_step = args.crops
    else:
        # configs[1]: this rank's 64-crop shard (seeds rank*B .. rank*B+B-1), resident in HBM; one forward per step
        img = synth.normalize_crops(synth.crops_u8(B, seed0=rank * B)).to(dev)
        ctxs = eng.contexts(B, nfl)
        nstep = [0]

        def step():
            c = ctxs[nstep[0] % nfl]                       # every step is one whole batch; steps alternate between the contexts
            nstep[0] += 1
            with torch.cuda.stream(c.stream):
                eng.forward(img, c.out, workspace=c.workspace)
                if shard._multi():        # N > 1 (or the HAMER_RCCL_AT_WORLD1=1 opt-in on one GPU): RCCL gather of the MANO parameters
                    shard.gather_mano(shard.pack_mano(c.out), dst=0)
            return c.out
        units_per_step = world * B
    torch.cuda.synchronize()

    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    last = None
    for _ in range(args.steps):
        last = step()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([elapsed], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    if args.workload == "shard1024":
        if rank == 0:
            assert last.shape == (args.crops, shard.PARAMS_PER_HAND) and torch.isfinite(last).all()
    else:
        for c in ctxs:
            assert torch.isfinite(c.out["pred_vertices"]).all()
    if args.dump_outputs and rank == 0:
        # shard1024: the gathered [rotmats(144) | betas(10) | cam(3)] rows of the whole job; crops: this rank's forward outputs
        dump_outputs(args.dump_outputs, {"mano_params": last} if args.workload == "shard1024" else last)

    res = None
    if rank == 0:
        hands = units_per_step * args.steps
        fl = flops_per_hand(cfg)
        if args.dtype == "fp8":
            workload = ("BASELINE configs[4]: batch=%d synthetic 256x256 crops per GPU, HaMeR ViT-H/16 with qkv/proj/fc1/fc2 in e4m3 on "
                        "the block-scaled fp8 MFMA (MXFP8 activations), attention bf16, fp32 residual, decoder and MANO, crops resident in HBM" % B)
        elif args.workload == "shard1024":
            workload = ("BASELINE configs[3]: %d synthetic 256x256 crops sharded over %d GPU(s) (ceil(n/N) each, forwards of %d), "
                        "HaMeR ViT-H/16 + decoder + MANO, RCCL gather of MANO parameters to rank 0" % (args.crops, world, B))
        else:
            workload = ("BASELINE configs[1]: batch=%d synthetic 256x256 crops per GPU, HaMeR ViT-H/16 + 6-layer decoder + MANO, "
                        "16-bit MFMA (%s operands), crops resident in HBM" % (B, args.dtype))
        res = {
            "metric": "hands/sec (HaMeR ViT-H/16 + decoder + MANO forward; detector bypassed)",
            "value": round(hands / elapsed, 2), "unit": "hands/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(1e3 * elapsed / args.steps, 4), "higher_is_better": True,
            "scaling": "strong" if args.workload == "shard1024" else "weak", "vs_baseline": None, "dtype": args.dtype, "data": "synthetic",
            "config": {"workload": workload, "batch_per_gpu": B, "global_batch": units_per_step, "batches_in_flight": nfl,
                       "weights": "seeded random-init fp32 master weights, rounded to the operand type at load",
                       "parallelism": f"crop-shard x{world}", "mfma_gflop_per_hand": round(fl["total_mfma"] / 1e9, 2)},
            "model_mfma_frac": round(hands / elapsed * fl["total_mfma"] / 1e12 / (PEAK_BF16_TFLOPS * world), 4),
        }
        if args.token_merge:                # tokens are merged away block by block: the dense model's FLOP count does not apply
            res["config"]["workload"] += "; ToMe token merging, r = (8, -1): tokens per crop after each block " + str(tome_tokens(eng))
            res["config"]["mfma_gflop_per_hand"] = None
            res["model_mfma_frac"] = None
        img = img if args.workload != "shard1024" else mine[:B].contiguous()

    # ---- roofline of the dominant kernel (the MFMA GEMM), HIP events on the launch stream
    if rank == 0 and args.full and not args.no_roofline:
        nprof = min(args.steps, 5)
        with L.profile(capacity=nprof * 512) as prof:
            for _ in range(nprof):
                eng.forward(img, out)                   # one stream: every launch timed alone, nothing overlapping it
            torch.cuda.synchronize()
        by_kind, gemm_fl, gemm_ms, per = {}, 0.0, 0.0, {}
        for kind, epi, M, N, K, ms in prof.records:
            by_kind[kind] = by_kind.get(kind, 0.0) + ms
            if kind == "gemm":
                gemm_fl += 2.0 * M * N * K
                gemm_ms += ms
                e = per.setdefault(EPI_NAMES[epi], [0, 0.0, 0.0])
                e[0] += 1; e[1] += ms; e[2] += 2.0 * M * N * K
        n_gemm = sum(v[0] for v in per.values())
        achieved = gemm_fl / (gemm_ms * 1e-3) / 1e12
        # HBM-side bytes per GEMM launch from the committed PMC pass (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE in separate
        # runs over tools/pmc_shapes.py, gfx950 FETCH_SIZE x2 correction; tools/pmc_parse.py), weighted by launches per step
        traffic, traffic_src = None, latest_profile("pmc_traffic.json")
        if traffic_src is not None and B == 64:
            t = json.load(open(traffic_src))
            w = {"patch": 1, "qkv": cfg.vit.depth, "proj": cfg.vit.depth, "fc1": cfg.vit.depth, "fc2": cfg.vit.depth, "kv": 1}
            traffic = round(sum(t[k]["hbm_bytes"] * n for k, n in w.items()) / sum(w.values()))
        kernel_name, peak = "gemm_px_kernel / gemm_x3_kernel / gemm_tn_kernel (the 256x256 MFMA GEMM, all epilogues)", PEAK_BF16_TFLOPS
        if args.dtype == "fp8":      # dominant kernel = gemm_fp8_kernel: price its launches against the fp8 peak
            f8 = [(M_, N_, K_, ms_) for (kd, e_, M_, N_, K_, ms_) in prof.records if kd == "gemm" and e_ >= 16]
            achieved = sum(2.0 * a * b * c for a, b, c, _ in f8) / (sum(t for *_, t in f8) * 1e-3) / 1e12
            kernel_name, peak, traffic = "gemm_fp8p_kernel (store / gelu_mx8) + gemm_fp8_kernel (resid_f32)", PEAK_FP8_TFLOPS, None
        res["roofline"] = {
            "kernel": kernel_name, "bound": "mfma", "achieved": round(achieved, 2),
            "peak": peak, "unit": "TFLOP/s", "frac": round(achieved / peak, 4), "traffic": traffic,
            "traffic_note": "bytes per launch beyond L2 (FETCH_SIZE*2 + WRITE_SIZE, PMC pass %s; Infinity-Cache hits included), " % (os.path.basename(traffic_src) if traffic_src else "absent") +
                            "algorithmic operand+result bytes per launch: %d" % round(sum(
                                (2 * (M_ * K_ + N_ * K_) + M_ * N_ * {2: 8, 5: 10}.get(e_, 2)) for (_, e_, M_, N_, K_, _) in
                                [r for r in prof.records if r[0] == "gemm"]) / n_gemm),
            "mfma_busy_pmc": mfma_busy_pmc(cfg) if (B == 64 and args.dtype != "fp8") else None,
            "launches_per_step": n_gemm // nprof, "avg_launch_ms": round(gemm_ms / n_gemm, 5),
            "flop_per_launch": round(gemm_fl / n_gemm),
            "per_epilogue": {k: {"launches_per_step": v[0] // nprof, "avg_ms": round(v[1] / v[0], 5),
                                 "tflops": round(v[2] / (v[1] * 1e-3) / 1e12, 2)} for k, v in per.items()},
            "ms_per_step_by_kernel": {k: round(v / nprof, 4) for k, v in sorted(by_kind.items(), key=lambda kv: -kv[1])},
            "timing": f"hipEvent pairs around every launch, separate pass of {nprof} steps after the timed region",
        }
    if rank == 0 and shard.FORCE_COLLECTIVES:
        res["config"]["rccl_at_world1"] = "HAMER_RCCL_AT_WORLD1=1: weight broadcast and per-step MANO gather ran through RCCL on one rank"
    default_line = (world == 1 and not shard.FORCE_COLLECTIVES and args.workload == "crops" and args.dtype == "fp16" and B == 64 and not args.token_merge
                    and not args.fold_ln and args.gemm_variant < 0)
    if rank == 0 and args.full and default_line and not args.no_side:
        res["side_configs"] = side_configs(args, dev, cfg, sd, mano_cpu, eng, res["value"], ctxs)
    if rank == 0 and args.full and world == 1 and not args.no_cpu_baseline:
        res["cpu_baseline"] = cpu_baseline(cfg, sd, mano_cpu)
    if dist.is_initialized():
        dist.barrier()
        shard.shutdown_distributed()
    if rank == 0:
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
