"""GPU: the precise (fp32) YOLOv7 route -- ``Detector(config, precise=True)``, ``YoloEngine(dtype=torch.float32)``, HM_DTYPE_F32.

It is the reference's CPU branch (yolo/detector.py:110-112 with ``half = False``): fp32 image, weights and activations, the
convolutions on the fp32-input MFMA (conv_f32.hip: each output = bias + a sum over K in one order fixed by K, so it is
deterministic and batch-invariant), pooling, upsampling and letterbox exact.  The oracle is ``oracle/yolo_ref`` with
``emu=False``.  Measured levels are printed, appended as JSON lines to the file named by $HAMER_PARITY_REPORT when it is set,
and recorded in DESIGN.md."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exact_data as ED  # noqa: E402

from hamer_yolo_amd import lib as L
from hamer_yolo_amd import synth
from hamer_yolo_amd.yolo import arch, fuse
from hamer_yolo_amd.yolo.detector import Detector
from hamer_yolo_amd.yolo.engine import YoloEngine
from oracle import yolo_ref

DEV = "cuda"
YOLO_SPEC = "synthetic:2:-2.2:0"      # ~10 boxes of both labels per seeded 1080p frame (as tests/test_gpu_chain.py)
SEEDS = (0, 1, 2, 3, 4, 5)


class _YCfg:
    weights = YOLO_SPEC; imgsz = 640; augment = True; conf_thres = 0.25; iou_thres = 0.35
    classes = [0, 1, 2]; agnostic_nms = True; device = "cuda"; save_path = "./output"


class _YCfgPrecise(_YCfg):
    precise = True


def _report(rep):
    """Print the measured levels; also append them to $HAMER_PARITY_REPORT (a JSON-lines file) when that is set."""
    print(rep)
    path = os.environ.get("HAMER_PARITY_REPORT")
    if not path:
        return
    try:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "a") as f:
            f.write(json.dumps(rep) + "\n")
    except OSError:
        pass


def _ulp(v):
    return torch.from_numpy(np.spacing(np.abs(v.float().numpy())).astype(np.float64))


# ------------------------------------------------------------------ 1. the convolution
def _conv_f32(x, w, b, k, s, act, ld_extra=0, y_extra=0):
    """hm_conv2d_nhwc with HM_DTYPE_F32 on an NHWC copy of x (input and output as channel slices of wider buffers when
    ld_extra / y_extra are given; the neighbouring channels of the output must stay untouched)."""
    lib = L.load()
    N, Ci, H, W = x.shape
    Co = w.shape[0]
    cin = 8 if Ci < 8 else Ci
    xb = torch.zeros(N, H, W, cin + ld_extra)
    xb[..., ld_extra:ld_extra + Ci] = x.permute(0, 2, 3, 1)
    wk = torch.zeros(Co, k, k, cin)
    wk[..., :Ci] = w.permute(0, 2, 3, 1)
    kp = (k * k * cin + 63) // 64 * 64
    wf = torch.zeros(Co, kp)
    wf[:, :k * k * cin] = wk.reshape(Co, -1)
    Ho, Wo = (H + 2 * (k // 2) - k) // s + 1, (W + 2 * (k // 2) - k) // s + 1
    xd, wd, bd = xb.to(DEV), wf.to(DEV), b.float().to(DEV)
    yd = torch.full((N, Ho, Wo, Co + 2 * y_extra), 7.0, device=DEV)
    a = L.ConvArgs(xd.data_ptr() + ld_extra * 4, wd.data_ptr(), yd.data_ptr() + y_extra * 4, bd.data_ptr(), None, N, H, W, cin, Co,
                   k, s, cin + ld_extra, Co + 2 * y_extra, kp, int(act), 0, L.HM_DTYPE_F32, None, 0, None, 0)
    L.check(lib.hm_conv2d_nhwc(C.byref(a), L.current_stream()), "hm_conv2d_nhwc")
    torch.cuda.synchronize()
    y = yd.cpu()
    assert (y[..., :y_extra] == 7.0).all() and (y[..., y_extra + Co:] == 7.0).all()      # neighbours untouched
    return y[..., y_extra:y_extra + Co].permute(0, 3, 1, 2).contiguous()


# the shapes of test_gpu_yolo.py::test_conv2d_nhwc_vs_torch (K up to 4608), a 1024 -> 24 detect head, a Cout that is no multiple
# of 32, and maps large enough for the 128 x 128 tile (the one-frame maps take 64 x 64: the tile never changes a result)
SHAPES = [(3, 32, 3, 1, 40, 72, 2), (32, 64, 3, 2, 38, 70, 2), (64, 64, 1, 1, 24, 40, 2), (128, 256, 3, 1, 12, 20, 2),
          (256, 24, 1, 1, 12, 20, 2), (64, 128, 3, 2, 31, 33, 2), (512, 512, 3, 1, 6, 10, 2), (1024, 24, 1, 1, 12, 20, 2),
          (64, 40, 3, 1, 17, 23, 1), (64, 256, 1, 1, 96, 160, 2)]


@pytest.mark.parametrize("Ci,Co,k,s,H,W,N", SHAPES)
def test_conv_f32_within_the_fp32_summation_bound(Ci, Co, k, s, H, W, N):
    """|got - exact| <= 1e-6 * sum|x * w| on the pre-activation (the guide measures 0.75-3.5e-7 * sum|a * b| for fp32 MFMA at
    K <= 4096), plus 4 ulp of the output where SiLU follows.  The exact value and sum|x * w| are float64 convolutions."""
    x = synth.uniform("cx", (N, Ci, H, W), 1.0, seed=Ci)
    w = synth.uniform("cw", (Co, Ci, k, k), (3.0 / (Ci * k * k)) ** 0.5, seed=Co)
    b = synth.uniform("cb", (Co,), 0.3, seed=k)
    ref = F.conv2d(x.double(), w.double(), b.double(), stride=s, padding=k // 2)
    mag = F.conv2d(x.double().abs(), w.double().abs(), b.double().abs(), stride=s, padding=k // 2)
    y = _conv_f32(x, w, b, k, s, act=False)
    err = (y.double() - ref).abs()
    assert bool((err <= 1e-6 * mag).all()), float((err / mag).max())
    y = _conv_f32(x, w, b, k, s, act=True, ld_extra=8 if Ci >= 8 else 0, y_extra=8)
    ref_s = F.silu(ref)
    err_s = (y.double() - ref_s).abs()
    assert bool((err_s <= 1.1e-6 * mag + 4 * _ulp(ref_s)).all()), float((err_s - 1.1e-6 * mag).max())


def test_conv_f32_exact_integer_data_bit_equal():
    """Hashed integers (tests/exact_data.py): exact in fp32 whatever the summation order, and no two operand elements alike
    along any axis (tests/test_exact_data_host.py lists the index faults that data sees)."""
    for (n, Ci, Co, k, s, H, W) in ED.CONV_F32:
        x, w, b = ED.conv_case(n, Ci, Co, k, H, W)
        ref = F.conv2d(x, w, b, stride=s, padding=k // 2)
        ED.assert_exact(_conv_f32(x, w, b, k, s, act=False), ref, (Ci, Co, k, s))


# ------------------------------------------------------------------ 2. determinism and batch invariance
@pytest.fixture(scope="module")
def engine32():
    return YoloEngine(synth.yolo_state_dict(seed=0, nc=3), nc=3, device=DEV, dtype=torch.float32)


def test_fp32_route_is_deterministic_and_batch_invariant(engine32):
    eng = engine32
    assert eng.dt == L.HM_DTYPE_F32 and not eng.split_k and not eng.fuse_stem
    frames = [synth.frame_u8(1080, 1920, seed=40 + i).to(DEV) for i in range(3)]
    p = eng.forward(frames)
    first = p["pred"].clone()
    p = eng.forward(frames)
    torch.cuda.synchronize()
    assert torch.equal(p["pred"], first)                                  # two runs: the same bytes
    n = p["n_pred"]
    for i, f in enumerate(frames):                                        # three single passes: the same bytes
        assert torch.equal(eng.forward(f)["pred"], first[i * n:(i + 1) * n]), i
    stacked = torch.stack(frames)                                          # slices of one tensor: the one-launch letterbox
    ps = eng.forward([stacked[i] for i in range(3)])
    torch.cuda.synchronize()
    assert torch.equal(ps["pred"], first)
    ps = eng.forward([stacked[2], stacked[0]])                             # another pass size, other positions
    torch.cuda.synchronize()
    assert torch.equal(ps["pred"][:n], first[2 * n:]) and torch.equal(ps["pred"][n:], first[:n])


# ------------------------------------------------------------------ 3. small ops
def test_fp32_maxpool_and_upsample_exact():
    lib = L.load()
    F32 = L.HM_DTYPE_F32
    for n, Cc, Hh, Ww, k, s, pad in ((3, 128, 16, 24, 2, 2, 0), (2, 64, 10, 14, 2, 2, 0), (1, 64, 7, 9, 2, 2, 0),
                                     (2, 64, 12, 20, 5, 1, 2), (1, 64, 15, 11, 3, 2, 1)):
        xs = synth.uniform("mp", (n, Cc, Hh, Ww), 2.0, seed=Hh)
        xb = torch.zeros(n, Hh, Ww, Cc + 64)
        xb[..., 32:32 + Cc] = xs.permute(0, 2, 3, 1)
        xbd = xb.to(DEV)
        Ho, Wo = (Hh + 2 * pad - k) // s + 1, (Ww + 2 * pad - k) // s + 1
        yb = torch.full((n, Ho, Wo, Cc + 32), 3.0, device=DEV)
        L.check(lib.hm_maxpool_nhwc(xbd.data_ptr() + 32 * 4, Cc + 64, yb.data_ptr() + 16 * 4, Cc + 32, n, Hh, Ww, Cc, k, s, pad,
                                    F32, L.current_stream()))
        got = yb.cpu()
        assert torch.equal(got[..., 16:16 + Cc].permute(0, 3, 1, 2), F.max_pool2d(xs, k, s, pad)), (n, Cc, Hh, Ww, k)
        assert (got[..., :16] == 3.0).all() and (got[..., 16 + Cc:] == 3.0).all()
    # SPPCSPC: 5, 9 = 5o5, 13 = 5o5o5 into channel slices of one buffer
    x = synth.uniform("px", (1, 64, 12, 20), 2.0, seed=1)
    cat = torch.zeros(1, 12, 20, 256, device=DEV)
    cat[..., :64] = x.permute(0, 2, 3, 1).to(DEV)
    for step in range(3):
        L.check(lib.hm_maxpool_nhwc(cat.data_ptr() + step * 256, 256, cat.data_ptr() + (step + 1) * 256, 256, 1, 12, 20, 64, 5, 1, 2,
                                    F32, L.current_stream()))
    ref = torch.cat([x] + [F.max_pool2d(x, k, 1, k // 2) for k in (5, 9, 13)], 1)
    assert torch.equal(cat.cpu().permute(0, 3, 1, 2), ref)
    xd = torch.zeros(2, 12, 20, 96, device=DEV)
    xd[..., 16:80] = torch.cat([x, -x]).permute(0, 2, 3, 1).to(DEV)
    up = torch.full((2, 24, 40, 80), 5.0, device=DEV)
    L.check(lib.hm_upsample2x_nhwc(xd.data_ptr() + 16 * 4, 96, up.data_ptr() + 8 * 4, 80, 2, 12, 20, 64, F32, L.current_stream()))
    got = up.cpu()
    assert torch.equal(got[..., 8:72].permute(0, 3, 1, 2), F.interpolate(torch.cat([x, -x]), scale_factor=2, mode="nearest"))
    assert (got[..., :8] == 5.0).all() and (got[..., 72:] == 5.0).all()


@pytest.mark.parametrize("hw", [(1080, 1920), (565, 848), (384, 640), (700, 500)])
def test_fp32_letterbox_bit_exact(engine32, hw):
    """x8 = the oracle's letterbox(...) -> torch .float() / 255.0, bit for bit (an IEEE division, as torch's)."""
    frame = synth.frame_u8(hw[0], hw[1], seed=hw[0])
    p = engine32.letterbox(frame.to(DEV), want_u8=True)
    torch.cuda.synchronize()
    ref, _ = yolo_ref.letterbox(frame.numpy())
    assert np.array_equal(p["u8"].cpu().numpy(), ref)
    lp = p["lp"]
    off = p["img_ptr"] - p["arena"].data_ptr()
    x8 = p["arena"][off:off + lp.out_h * lp.out_w * 32].view(torch.float32).reshape(lp.out_h, lp.out_w, 8).cpu()
    assert torch.equal(x8[..., :3].permute(2, 0, 1), torch.from_numpy(ref).float() / 255.0)
    assert (x8[..., 3:] == 0).all()
    # the batched letterbox writes the same bytes
    stacked = torch.stack([frame, frame.flip(0).contiguous()]).to(DEV)
    pb = engine32._plan(hw[0], hw[1], 2)
    L.check(engine32.lib.hm_letterbox_batch(stacked.data_ptr(), stacked[1].data_ptr() - stacked[0].data_ptr(), 2, C.byref(pb["lp"]),
                                            pb["tab"].data_ptr(), pb["img_ptr"], L.HM_DTYPE_F32, L.current_stream()))
    torch.cuda.synchronize()
    offb = pb["img_ptr"] - pb["arena"].data_ptr()
    xb = pb["arena"][offb:offb + lp.out_h * lp.out_w * 32].view(torch.float32).reshape(lp.out_h, lp.out_w, 8).cpu()
    assert torch.equal(xb, x8)


# ------------------------------------------------------------------ 4. every layer, teacher-forced
def _fused(seed=0, **kw):
    layers = arch.yolov7_layers()
    return layers, fuse.fuse_state_dict(synth.yolo_state_dict(seed=seed, nc=3, **kw), arch.conv_specs(layers, 3, 3))


def test_every_layer_fp32_vs_oracle_on_the_gpus_own_inputs(engine32):
    """Each layer of the fp32 network recomputed by yolo_ref.layer_forward(emu=False) -- in float64, so what is left is the GPU's
    own error -- from the GPU's own input tensors of that layer.  mp / up / concat exact; a convolution within the bound of
    test 1 (1.1e-6 * sum|x * w| + 4 ulp after SiLU; SPPCSPC's seven convolutions and three pools teacher-forced one by one
    from its scratch buffers in the arena); detect heads rtol 1e-5 + 1e-6 * sum|x * w|."""
    torch.set_num_threads(max(1, min(16, len(os.sched_getaffinity(0)))))
    frame = synth.frame_u8(540, 960, seed=5)
    p = engine32.forward(frame.to(DEV))
    torch.cuda.synchronize()
    layers, fused = _fused()
    f64 = {k: (w.double(), b.double()) for k, (w, b) in fused.items()}
    fabs = {k: (w.double().abs(), b.double().abs()) for k, (w, b) in fused.items()}
    lp = p["lp"]
    off = p["img_ptr"] - p["arena"].data_ptr()
    x8 = p["arena"][off:off + lp.out_h * lp.out_w * 32].view(torch.float32).reshape(lp.out_h, lp.out_w, 8).cpu()
    img = x8[..., :3].permute(2, 0, 1)[None].contiguous()
    outs = {}
    get = lambda j: outs.setdefault(j, engine32.layer_output(p, j)[None])
    worst = {"conv": 0.0, "sppcspc": 0.0, "detect": 0.0}
    n_conv = 0

    def check_conv(name, x, got, k, s, key):
        """got (1, C, H, W) against the float64 conv + SiLU of the GPU's own input x"""
        w, b = f64[name]
        ref = F.silu(F.conv2d(x, w, b, stride=s, padding=k // 2))
        mag = F.conv2d(x.abs(), fabs[name][0], fabs[name][1], stride=s, padding=k // 2)
        err = (got - ref).abs()
        assert bool((err <= 1.1e-6 * mag + 4 * _ulp(ref)).all()), (name, float((err - 1.1e-6 * mag).max()))
        worst[key] = max(worst[key], float((err / mag).max()))

    def spp_buf(j, cc, c0, c1, hw):
        """channels [c0, c1) of SPPCSPC scratch buffer j (1000..1004, see YoloEngine._plan) as (1, C, H, W) float64"""
        h, w = hw
        t = p["arena"][p["offs"][j]:p["offs"][j] + h * w * cc * 4].view(torch.float32).reshape(h, w, cc)
        return t[:, :, c0:c1].permute(2, 0, 1)[None].double().cpu()
    with torch.no_grad():
        for i, (srcs, kind, args) in enumerate(arch.resolve(layers)):
            inp = [(img if s < 0 else get(s)).double() for s in srcs]
            ref = yolo_ref.layer_forward(layers, f64, i, inp, 3, emu=False)
            if kind == "detect":
                for l, ((raw, hh, ww), r) in enumerate(zip(p["raws"], ref)):
                    mine = raw.cpu().double().reshape(hh, ww, 3, 8).permute(2, 0, 1, 3)
                    w_, b_ = fabs[f"model.{i}.m.{l}"]
                    mag = F.conv2d(inp[l].abs(), w_, b_).view(3, 8, hh, ww).permute(0, 2, 3, 1)
                    err = (mine - r[0]).abs()
                    bound = 1e-5 * r[0].abs() + 1e-6 * mag
                    assert bool((err <= bound).all()), (l, float((err - bound).max()))
                    worst["detect"] = max(worst["detect"], float((err / mag).max()))
                continue
            got = get(i).double()
            assert got.shape == ref.shape, (i, kind, got.shape, ref.shape)
            if kind in ("mp", "up", "concat"):
                assert torch.equal(got, ref), (i, kind)
                continue
            n_conv += 1
            if kind == "sppcspc":                                 # common.py:279-284, teacher-forced inside
                c_, hw = args[0], p["hw"][i]
                t1, t3, t5 = (spp_buf(j, c_, 0, c_, hw) for j in (1000, 1001, 1003))
                cat4 = [spp_buf(1002, 4 * c_, q * c_, (q + 1) * c_, hw) for q in range(4)]
                cat2 = [spp_buf(1004, 2 * c_, q * c_, (q + 1) * c_, hw) for q in range(2)]
                pre = f"model.{i}."
                check_conv(pre + "cv1.conv", inp[0], t1, 1, 1, "sppcspc")
                check_conv(pre + "cv3.conv", t1, t3, 3, 1, "sppcspc")
                check_conv(pre + "cv4.conv", t3, cat4[0], 1, 1, "sppcspc")
                for q in range(3):                                # 5, 9 = 5o5, 13 = 5o5o5: exact
                    assert torch.equal(cat4[q + 1], F.max_pool2d(cat4[q], 5, 1, 2)), q
                check_conv(pre + "cv5.conv", torch.cat(cat4, 1), t5, 1, 1, "sppcspc")
                check_conv(pre + "cv6.conv", t5, cat2[0], 3, 1, "sppcspc")
                check_conv(pre + "cv2.conv", inp[0], cat2[1], 1, 1, "sppcspc")
                check_conv(pre + "cv7.conv", torch.cat(cat2, 1), got, 1, 1, "sppcspc")
                continue
            name = f"model.{i}.conv" if kind == "conv" else f"model.{i}.rbr_reparam"
            k, s = (args[1], args[2]) if kind == "conv" else (3, 1)
            check_conv(name, inp[0], got, k, s, "conv")
            assert torch.equal(F.silu(F.conv2d(inp[0], *f64[name], stride=s, padding=k // 2)), ref)     # = layer_forward
    assert n_conv == 79 + 3 + 1
    _report({"test": "yolo_fp32_every_layer_teacher_forced", "max_err_over_sum_abs_conv": worst["conv"],
             "max_err_over_sum_abs_sppcspc": worst["sppcspc"], "max_err_over_sum_abs_detect": worst["detect"]})


# ------------------------------------------------------------------ 5-7. the whole network, the boxes, end to end
@pytest.fixture(scope="module")
def oracle6():
    """yolo_ref.detect(emu=False) -- the reference's CPU detector -- on the six seeded 1080p frames: (dets, list, pred)."""
    torch.set_num_threads(max(1, min(16, len(os.sched_getaffinity(0)))))
    layers, fused = _fused(seed=2, obj_bias=-2.2, cls_bias=0.0)
    out = {}
    with torch.no_grad():
        for seed in SEEDS:
            fr = synth.frame_u8(1080, 1920, seed=seed).numpy()
            out[seed] = (fr,) + tuple(yolo_ref.detect(layers, fused, fr, 3, arch.ANCHORS, emu=False))
    return out


@pytest.fixture(scope="module")
def det32():
    return Detector(_YCfg, precise=True)


@pytest.fixture(scope="module")
def det16():
    return Detector(_YCfg)


def _pred_of(det, fr):
    det.detect(fr)
    return det.engine._plan(fr.shape[0], fr.shape[1])["pred"].cpu()


def test_whole_network_fp32_pred_vs_the_fp32_oracle(det32, det16, oracle6):
    """The fp32 route's pred against yolo_ref.detect(emu=False)'s on the six frames: confidence / class columns within 1e-5,
    xywh within 1e-2 letterbox px; and at least 100x closer than the fp16 route on the same frames (the test tells the two
    routes apart).  Measured on the MI355X: fp32 route 9.5e-4 px / 4.6e-6, fp16 route 0.36 px / 2.5e-3."""
    e32 = {"xywh": 0.0, "score": 0.0}
    e16 = {"xywh": 0.0, "score": 0.0}
    for seed in SEEDS:
        fr, _, _, ref = oracle6[seed]
        ref = ref[0]
        for det, e in ((det32, e32), (det16, e16)):
            d = (_pred_of(det, fr) - ref).abs()
            e["xywh"] = max(e["xywh"], float(d[:, :4].max()))
            e["score"] = max(e["score"], float(d[:, 4:].max()))
    _report({"test": "yolo_fp32_pred_vs_fp32_oracle", "frames": len(SEEDS), "fp32_max_xywh_px": e32["xywh"],
             "fp32_max_score": e32["score"], "fp16_max_xywh_px": e16["xywh"], "fp16_max_score": e16["score"]})
    assert e32["score"] <= 1e-5 and e32["xywh"] <= 1e-2, e32
    assert e16["score"] >= 100 * e32["score"] and e16["xywh"] >= 100 * e32["xywh"], (e16, e32)


def test_boxes_equal_the_fp32_cpu_detector(det32, oracle6):
    """Detector(cfg, precise=True).detect gives the fp32 oracle detector's box list exactly: count, order, labels, rounded
    corners.  Exempt only a declared tie: a corner whose unrounded oracle value (NMS + scale_coords on the oracle pred,
    before .round()) lies within 0.02 px of a half-integer; at most 2 over the six frames.  detect_frames on the six frames
    returns what six detect calls return."""
    geo = yolo_ref.letterbox_geometry(1080, 1920)
    n_boxes = ties = near_half = 0
    singles = []
    for seed in SEEDS:
        fr, _, ref_list, ref_pred = oracle6[seed]
        pred, got = det32.detect(fr)
        singles.append((pred[0].cpu(), got[0]))
        want = ref_list[0]
        assert len(got[0]) == len(want), (seed, len(got[0]), len(want))
        x = yolo_ref.non_max_suppression(ref_pred.clone(), 0.25, 0.35, [0, 1, 2], True)[0]
        unr = yolo_ref.scale_coords((geo["out_h"], geo["out_w"]), x[:, :4].clone(), fr.shape)
        assert len(unr) == len(want)
        for j, ((lg, bg), (lw, bw)) in enumerate(zip(got[0], want)):
            assert lg == lw, (seed, j)
            for c in range(4):
                u = float(unr[j, c])
                is_tie = abs(abs(u - np.floor(u)) - 0.5) < 0.02
                near_half += int(is_tie)
                if bg[c] != bw[c]:
                    assert is_tie and abs(bg[c] - bw[c]) == 1.0, (seed, j, c, bg, bw, u)
                    ties += 1
        n_boxes += len(want)
    _report({"test": "yolo_fp32_boxes_vs_fp32_cpu_detector", "frames": len(SEEDS), "boxes": n_boxes, "corner_ties_exempted": ties,
             "corners_within_0.02_of_half": near_half})
    assert n_boxes >= 30 and ties <= 2
    frames = [torch.from_numpy(oracle6[s][0]).to(DEV) for s in SEEDS]
    preds, lists = det32.detect_frames(frames)
    for (p1, l1), p2, l2 in zip(singles, preds, lists):
        assert torch.equal(p1, p2.cpu()) and l1 == l2


def _rotvec(Rm):
    from scipy.spatial.transform import Rotation
    return Rotation.from_matrix(np.asarray(Rm, dtype=np.float64).reshape(-1, 3, 3)).as_rotvec().astype(np.float32)


def _oracle_record(frame, det, sd, mp, cfg):
    """infer.py:1268-1303 for one hand with k_real = None: crop -> HaMeR (fp32 oracle) -> camera step -> record."""
    from oracle import crop_ref
    from oracle import hamer_ref as R
    mean = 255.0 * np.array([0.485, 0.456, 0.406]); std = 255.0 * np.array([0.229, 0.224, 0.225])
    batch = crop_ref.prepare_batch_bbox(frame, [det], mean, std)
    with torch.no_grad():
        o = R.hamer_forward(sd, mp, torch.from_numpy(batch["img"]), cfg)
    cam = o["pred_cam"][0].clone()
    cam[1] *= 1.0 - 2.0 * float(batch["do_flip"][0])
    H, W = frame.shape[:2]
    f = 5000.0 / 256.0 * max(H, W)                                   # infer.py:478-480
    bs = float(batch["box_size"][0]) * float(cam[0]) + 1e-9          # renderer.py:54-72
    cam_t = np.array([2 * (batch["box_center"][0][0] - W / 2.0) / bs + float(cam[1]),
                      2 * (batch["box_center"][0][1] - H / 2.0) / bs + float(cam[2]), 2 * f / bs], dtype=np.float32)
    Rm = torch.cat([o["global_orient"][0], o["hand_pose"][0]], 0).numpy()
    return {"betas": o["betas"][0].numpy(), "theta": _rotvec(Rm).reshape(-1), "cam_t": cam_t, "rotmats": Rm}


def test_end_to_end_against_the_all_fp32_pipeline(tmp_path, oracle6):
    """Four 1080p PNGs through process_batch_manopara with the precise detector: every saved record equals crop_ref ->
    hamer_ref (fp32) -> camera step driven by the fp32 ORACLE detector's own boxes (betas and rotations within 1e-3, cam_t
    rtol 2e-3) -- the whole reference CPU pipeline, detector included."""
    from PIL import Image
    from scipy.spatial.transform import Rotation
    from hamer_yolo_amd.infer import box_has_area, hamer_inference, process_batch_manopara

    class _HCfg:
        ckpt_path = "synthetic:0"; model_cfg = None; use_onnx = False; onnx_path = None

    in_dir, out_dir = tmp_path / "rgb", tmp_path / "out"
    in_dir.mkdir()
    names = {f"f{s}": s for s in SEEDS[:4]}
    for name, s in names.items():
        Image.fromarray(oracle6[s][0][:, :, ::-1]).save(in_dir / f"{name}.png")
    process_batch_manopara(str(in_dir), str(out_dir), None, hamer=hamer_inference(_HCfg), detector=Detector(_YCfg, precise=True),
                           frames_per_step=2)
    cfg = synth.HamerConfig()
    sd, mp = synth.hamer_state_dict(cfg, seed=0), synth.mano_params(seed=0)
    n_hands, d_beta, d_rot, d_theta = 0, 0.0, 0.0, 0.0
    for name, s in names.items():
        fr, _, ref_list, _ = oracle6[s]
        dets = [d for d in ref_list[0] if box_has_area(d)]
        if not dets:                                                   # no detection: no file (infer.py:1296-1310)
            assert not (out_dir / f"{name}.npy").exists(), name
            continue
        rec = np.load(out_dir / f"{name}.npy", allow_pickle=True).item()
        for label in ("left", "right"):
            idx = [i for i, d in enumerate(dets) if d[0] == label]
            if not idx:
                assert rec[label] is None
                continue
            got, want = rec[label], _oracle_record(fr, dets[idx[-1]], sd, mp, cfg)      # the last detection of a label wins
            n_hands += 1
            got_R = Rotation.from_rotvec(got["theta"].reshape(16, 3).astype(np.float64)).as_matrix()
            d_beta = max(d_beta, float(np.abs(got["betas"] - want["betas"]).max()))
            d_rot = max(d_rot, float(np.abs(got_R - want["rotmats"]).max()))
            d_theta = max(d_theta, float(np.abs(got["theta"] - want["theta"]).max()))
            np.testing.assert_allclose(got["betas"], want["betas"], atol=1e-3, rtol=0)
            np.testing.assert_allclose(got_R, want["rotmats"], atol=1e-3, rtol=0)
            np.testing.assert_allclose(got["cam_t"], want["cam_t"], rtol=2e-3, atol=2e-3)
    _report({"test": "yolo_fp32_end_to_end_vs_all_fp32_pipeline", "frames": len(names), "hands": n_hands, "max_dbeta": d_beta,
             "max_drotmat": d_rot, "max_dtheta_axis_angle": d_theta})
    assert n_hands >= 5


# ------------------------------------------------------------------ 8. the default is unchanged
def test_default_detector_is_the_fp16_route(det16):
    assert det16.precise is False and det16.engine.dtype == torch.float16 and det16.engine.dt == L.HM_DTYPE_F16
    assert det16.engine.split_k and det16.engine.fuse_stem
    d = Detector(_YCfgPrecise)                                          # config.precise is read when precise=None
    assert d.precise is True and d.engine.dtype == torch.float32 and d.engine.dt == L.HM_DTYPE_F32
    assert Detector(_YCfgPrecise, precise=False).precise is False
    with pytest.raises(ValueError):
        YoloEngine(synth.yolo_state_dict(seed=0, nc=3), nc=3, device=DEV, dtype=torch.float64)
