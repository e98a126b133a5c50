"""The SAR hand-mesh head's kernels (csrc/sar.hip, csrc/sar_f32.hip) on exact data, bit for bit.

GEMM modes (hm_sar_saigb, hm_sar_saigb_ch, hm_sar_graph_mix, hm_sar_linear and the three *_f32 twins): hashed small-integer
operands (tests/exact_data.py), so every product and partial sum is an integer below 2^24 and every fp16 output an fp16 value
but for the one rounding of the LeakyReLU's negative half, which the reference states as one fp32 multiply and one
round-to-nearest conversion.  Shapes reach the half N tile, the row and column clamps, the k rows past 778 (NaN in memory),
one K step, an odd number of K steps and Laplacian strides that add K steps of zeros.  Outputs start as NaN; sentinel rows
come back untouched.

hm_sar_softargmax: few-hot logits whose softmax is 1 / m on a hashed support and exactly 0 elsewhere (or uniform where
beta = 0), so all 799 coordinates per hand have a closed form that is an fp32 value; dense integer mesh2pose weights pin the
in-place joint logits bit for bit, one-hot ones pin the joint coordinates.

hm_sar_postprocess: dyadic coordinates, transforms, roots, camera and depth maps, so uvd and xyz are exact whatever the
operation order or contraction; per-hand structs, flip, root source and depth sampling (inside, across a border, outside)
are all told apart.  tests/test_exact_data_host.py shows on the CPU that each data set sees its catalogue of faults.
"""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exact_data as ED  # noqa: E402

from hamer_yolo_amd import lib as L  # noqa: E402

DEV = "cuda"
NV, NJ, NT, CELLS, KG = ED.SAR_NV, ED.SAR_NJ, ED.SAR_NT, ED.SAR_CELLS, ED.SAR_KG
S_OUT = -12345.0
NAN = float("nan")


def _call(fn, *args):
    L.check(fn(*args, L.current_stream()), fn.__name__)


def _nan(shape, dtype):
    return torch.full(shape, NAN, dtype=dtype, device=DEV)


# ------------------------------------------------------------------------------------------------ SAIGB
@functools.lru_cache(maxsize=None)
def _saigb_case(B, K):
    return ED.sar_saigb_case(B, K)


@pytest.mark.parametrize("B,K", ED.SAR_SAIGB)
def test_saigb_exact(B, K):
    """The whole [778][B][544] graph -- 512 feature columns, 3 template columns, 29 zeros -- equals the reference bit for bit
    through hm_sar_saigb_ch (K = 512 and 1024) and, at K = 512, through hm_sar_saigb (the same bytes) and hm_sar_saigb_f32."""
    lib = L.load()
    feat, w, bias, tmpl, _, ref = _saigb_case(B, K)
    fh, wh, bd, td = feat.half().to(DEV), w.half().to(DEV), bias.to(DEV), tmpl.to(DEV)
    g = _nan((NV, B, KG), torch.float16)
    _call(lib.hm_sar_saigb_ch, L.ptr(fh), L.ptr(wh), L.ptr(bd), L.ptr(td), L.ptr(g), B, K)
    ED.assert_exact(g.reshape(NV * B, KG), ref["f16"].reshape(NV * B, KG), (B, K, "hm_sar_saigb_ch"))
    if K != 512:
        return
    g2 = _nan((NV, B, KG), torch.float16)
    _call(lib.hm_sar_saigb, L.ptr(fh), L.ptr(wh), L.ptr(bd), L.ptr(td), L.ptr(g2), B)
    ED.assert_exact(g2.reshape(NV * B, KG), ref["f16"].reshape(NV * B, KG), (B, K, "hm_sar_saigb"))
    assert torch.equal(g2.view(torch.int16), g.view(torch.int16))
    g3 = _nan((NV, B, KG), torch.float32)
    _call(lib.hm_sar_saigb_f32, L.ptr(feat.to(DEV)), L.ptr(w.to(DEV)), L.ptr(bd), L.ptr(td), L.ptr(g3), B)
    ED.assert_exact(g3.reshape(NV * B, KG), ref["f32"].reshape(NV * B, KG), (B, K, "hm_sar_saigb_f32"))


# ------------------------------------------------------------------------------------------------ L . X
def _mix(fn, dtype, lap, x, y_ref, N, ldl, what):
    """One launch: lap (778, ldl); x in an 800-row buffer whose rows 778 .. 799 hold NaN; y rows 0 .. 777 start as NaN and row
    778 is a sentinel."""
    xb = _nan((ED.SAR_MIX_XROWS, N), dtype)
    xb[:NV] = x.to(dtype)
    yb = _nan((NV + 1, N), dtype)
    yb[NV] = S_OUT
    ld = lap.to(dtype).to(DEV)
    assert ld.shape == (NV, ldl) and ld.is_contiguous()
    _call(fn, L.ptr(ld), ldl, L.ptr(xb), N, L.ptr(yb))
    ED.assert_exact(yb[:NV], y_ref.to(dtype), what)
    assert bool((yb[NV] == S_OUT).all()), what + ("sentinel row",)
    assert bool(xb[NV:].isnan().all()) and torch.equal(xb[:NV].cpu(), x.to(dtype))


@pytest.mark.parametrize("ldl", ED.SAR_MIX_LDL)
@pytest.mark.parametrize("N", ED.SAR_MIX_N + ED.SAR_MIX_N_F32_ONLY)
def test_graph_mix_exact(N, ldl):
    """lap[:, :778] x through hm_sar_graph_mix (f16, N % 8 == 0) and hm_sar_graph_mix_f32 (N % 4 == 0): the f16 kernel clamps
    the k rows past 777 to row 777 and the fp32 one loads zeros; the NaN stored there reaches neither result."""
    lib = L.load()
    lap, x, y = ED.sar_mix_case(N, ldl)
    if N not in ED.SAR_MIX_N_F32_ONLY:
        _mix(lib.hm_sar_graph_mix, torch.float16, lap, x, y, N, ldl, (N, ldl, "hm_sar_graph_mix"))
    _mix(lib.hm_sar_graph_mix_f32, torch.float32, lap, x, y, N, ldl, (N, ldl, "hm_sar_graph_mix_f32"))


# ------------------------------------------------------------------------------------------------ fc
@pytest.mark.parametrize("M,N,K", ED.SAR_FC)
def test_linear_exact(M, N, K):
    """hm_sar_linear with out_f32 = 0 (LeakyReLU, fp16) and 1 (raw fp32) and hm_sar_linear_f32 with logits = 0 (LeakyReLU) and 1:
    bit-equal, the output NaN beforehand, a sentinel row after row M - 1 (the row the M clamp re-reads) untouched."""
    lib = L.load()
    x, w, bias, ref = ED.sar_fc_case(M, N, K)
    bd = bias.to(DEV)
    runs = [(lib.hm_sar_linear, torch.float16, 0, torch.float16, "f16_leaky"), (lib.hm_sar_linear, torch.float16, 1, torch.float32, "f32"),
            (lib.hm_sar_linear_f32, torch.float32, 0, torch.float32, "f32_leaky"), (lib.hm_sar_linear_f32, torch.float32, 1, torch.float32, "f32_logits")]
    for fn, tin, flag, tout, key in runs:
        xd, wd = x.to(tin).to(DEV), w.to(tin).to(DEV)
        out = _nan((M + 1, N), tout)
        out[M] = S_OUT
        _call(fn, L.ptr(xd), M, K, L.ptr(wd), L.ptr(bd), L.ptr(out), N, flag)
        what = (M, N, K, fn.__name__, flag)
        assert ref[key].dtype == tout
        ED.assert_exact(out[:M], ref[key], what)
        assert bool((out[M] == S_OUT).all()), what + ("sentinel row",)


# ------------------------------------------------------------------------------------------------ soft-argmax
@functools.lru_cache(maxsize=None)
def _softargmax_run(B, m2p):
    """One hm_sar_softargmax launch on the case: (case, coords (B, 799, 3), joint logits xy, z (B, 21, 1024), the vertex rows of
    both logits buffers after the call), all on the CPU."""
    lib = L.load()
    c = ED.sar_softargmax_case(B, m2p)
    bufs = []
    for t in (c["lxy"], c["lz"]):
        buf = _nan((NT, B, CELLS), torch.float32)
        buf[:NV] = t.permute(1, 0, 2)
        bufs.append(buf)
    coords = _nan((B * NT * 3 + 3,), torch.float32)
    coords[B * NT * 3:] = S_OUT
    dev = {k: c[k].to(DEV).contiguous() for k in ("w_xy", "b_xy", "w_z", "b_z", "beta", "wx", "wy")}
    _call(lib.hm_sar_softargmax, L.ptr(bufs[0]), L.ptr(bufs[1]), L.ptr(dev["w_xy"]), L.ptr(dev["b_xy"]), L.ptr(dev["w_z"]),
          L.ptr(dev["b_z"]), L.ptr(dev["beta"]), L.ptr(dev["wx"]), L.ptr(dev["wy"]), L.ptr(coords), B)
    assert bool((coords[B * NT * 3:] == S_OUT).all())
    joints = [b[NV:].permute(1, 0, 2).cpu() for b in bufs]
    verts = [b[:NV].permute(1, 0, 2).cpu() for b in bufs]
    return c, coords[:B * NT * 3].reshape(B, NT, 3).cpu(), joints, verts


@pytest.mark.parametrize("B", ED.SAR_SOFTARGMAX_B)
def test_softargmax_dense_mesh2pose_exact(B):
    """Dense integer mesh2pose weights: rows 778 .. 798 of both logits buffers equal W logits + bias bit for bit and rows
    0 .. 777 are unchanged; the vertex coordinates equal the closed form bit for bit; the joint coordinates meet the float64
    softmax of the exact joint logits at test_softargmax_kernel's atol = 1e-5."""
    c, coords, joints, verts = _softargmax_run(B, "dense")
    ED.assert_exact(joints[0].reshape(B * NJ, CELLS), c["jxy"].reshape(B * NJ, CELLS), (B, "joint logits xy"))
    ED.assert_exact(joints[1].reshape(B * NJ, CELLS), c["jz"].reshape(B * NJ, CELLS), (B, "joint logits z"))
    assert torch.equal(verts[0], c["lxy"]) and torch.equal(verts[1], c["lz"])
    ED.assert_exact(coords[:, :NV].reshape(B * NV, 3), c["coords"][:, :NV].float().reshape(B * NV, 3), (B, "vertex coordinates"))
    np.testing.assert_allclose(coords[:, NV:].double().numpy(), c["coords"][:, NV:].numpy(), rtol=0, atol=1e-5)


@pytest.mark.parametrize("B", ED.SAR_SOFTARGMAX_B)
def test_softargmax_onehot_mesh2pose_exact(B):
    """One-hot mesh2pose weights: joint row j is vertex row v_j plus an integer, few-hot itself, and takes beta[778 + j] and the
    z bias: all 799 coordinates per hand equal the closed form bit for bit."""
    c, coords, joints, _ = _softargmax_run(B, "onehot")
    ED.assert_exact(joints[0].reshape(B * NJ, CELLS), c["jxy"].reshape(B * NJ, CELLS), (B, "joint logits xy"))
    ED.assert_exact(joints[1].reshape(B * NJ, CELLS), c["jz"].reshape(B * NJ, CELLS), (B, "joint logits z"))
    ED.assert_exact(coords.reshape(B * NT, 3), c["coords"].float().reshape(B * NT, 3), (B, "coordinates"))


# ------------------------------------------------------------------------------------------------ post-processing
def _hand_structs(hands):
    arr = (L.SarHand * len(hands))()
    for s, h in zip(arr, hands):
        for i, v in enumerate(np.asarray(h["t"], np.float32).reshape(6)):
            s.bb2img[i] = float(v)
        s.depth_box, s.flip = float(h["box"]), int(h["flip"])
        s.img_w, s.img_h = ED.SAR_POST_IMG
        if h["map"] is None:
            s.depth_offset, s.depth_w, s.depth_h = -1, 0, 0
        else:
            s.depth_offset, s.depth_w, s.depth_h = ED.SAR_POST_MAPS[h["map"]]
        s.fx, s.fy, s.fu, s.fv = ED.SAR_POST_K
    return torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(DEV)


@pytest.mark.parametrize("with_root,with_depth", [(True, True), (True, False), (False, True)], ids=["root+depth", "depth=NULL", "root=NULL"])
def test_postprocess_exact(with_root, with_depth):
    """B = 5 hands with their own transforms, depth boxes and roots, two flipped, three taking the root from one of two depth
    maps (row 778 inside, across a border, outside): uvd and xyz of all 799 rows equal the float64 formulas bit for bit; the
    outputs start as NaN and the sentinels behind B * 799 * 3 stay.  depth = NULL sends every hand to root[b]; root = NULL gives
    the hands without a map a root of 0."""
    lib = L.load()
    coords, depth, hands, uvd_ref, xyz_ref = ED.sar_post_case(with_root, with_depth)
    B, n = ED.SAR_POST_B, ED.SAR_POST_B * NT * 3
    assert C.sizeof(L.SarHand) * B == _hand_structs(hands).numel()
    root = torch.tensor([h["root"] for h in hands], dtype=torch.float32).to(DEV) if with_root else None
    dd = depth.to(DEV) if with_depth else None
    outs = []
    for _ in range(2):
        o = _nan((n + 3,), torch.float32)
        o[n:] = S_OUT
        outs.append(o)
    cd, hd = coords.to(DEV), _hand_structs(hands)
    _call(lib.hm_sar_postprocess, L.ptr(cd), L.ptr(hd), L.ptr(root), L.ptr(dd), L.ptr(outs[0]), L.ptr(outs[1]), B, ED.SAR_POST_P)
    ED.assert_exact(outs[0][:n].reshape(B * NT, 3), uvd_ref.reshape(B * NT, 3), (with_root, with_depth, "uvd"))
    ED.assert_exact(outs[1][:n].reshape(B * NT, 3), xyz_ref.reshape(B * NT, 3), (with_root, with_depth, "xyz"))
    assert bool((outs[0][n:] == S_OUT).all()) and bool((outs[1][n:] == S_OUT).all())
    assert torch.equal(cd.cpu(), coords)


# ------------------------------------------------------------------------------------------------ argument checks
def test_bad_arguments_are_refused():
    """Each call is refused with HipLibraryError before any launch; every other argument of the call is valid."""
    lib = L.load()
    s = L.current_stream()
    h = lambda *shape: torch.zeros(*shape, dtype=torch.float16, device=DEV)      # noqa: E731
    f = lambda *shape: torch.zeros(*shape, dtype=torch.float32, device=DEV)      # noqa: E731
    lap_h, x_h, y_h = h(NV, 832), h(800, 16), h(NV, 16)
    lap_f, x_f, y_f = f(NV, 832), f(800, 16), f(NV, 16)
    bias, tmpl = f(8 * NV), f(NV, 3)
    feat, w, g = h(64 + 1, 1024), h(8 * NV, 1024), h(NV, 1, KG)
    lx, lw, ly = f(4 + 1, 64), f(8, 64), f(4, 8)
    bad = {
        "graph_mix N % 8": lambda: lib.hm_sar_graph_mix(L.ptr(lap_h), 800, L.ptr(x_h), 12, L.ptr(y_h), s),
        "graph_mix ldl < 778": lambda: lib.hm_sar_graph_mix(L.ptr(lap_h), 768, L.ptr(x_h), 16, L.ptr(y_h), s),
        "graph_mix ldl % 32": lambda: lib.hm_sar_graph_mix(L.ptr(lap_h), 808, L.ptr(x_h), 16, L.ptr(y_h), s),
        "linear K % 32": lambda: lib.hm_sar_linear(L.ptr(x_h), 4, 48, L.ptr(lap_h), L.ptr(bias), L.ptr(y_h), 8, 0, s),
        "saigb_ch 768 channels": lambda: lib.hm_sar_saigb_ch(L.ptr(feat), L.ptr(w), L.ptr(bias), L.ptr(tmpl), L.ptr(g), 1, 768, s),
        "saigb_ch feat off by 2 bytes": lambda: lib.hm_sar_saigb_ch(L.ptr(feat) + 2, L.ptr(w), L.ptr(bias), L.ptr(tmpl), L.ptr(g), 1, 512, s),
        "graph_mix_f32 N % 4": lambda: lib.hm_sar_graph_mix_f32(L.ptr(lap_f), 800, L.ptr(x_f), 6, L.ptr(y_f), s),
        "graph_mix_f32 ldl % 4": lambda: lib.hm_sar_graph_mix_f32(L.ptr(lap_f), 802, L.ptr(x_f), 16, L.ptr(y_f), s),
        "linear_f32 logits = 2": lambda: lib.hm_sar_linear_f32(L.ptr(lx), 4, 64, L.ptr(lw), L.ptr(bias), L.ptr(ly), 8, 2, s),
        "linear_f32 x off by 4 bytes": lambda: lib.hm_sar_linear_f32(L.ptr(lx) + 4, 4, 64, L.ptr(lw), L.ptr(bias), L.ptr(ly), 8, 0, s),
    }
    for name, call in bad.items():
        with pytest.raises(L.HipLibraryError):
            L.check(call(), name)
    torch.cuda.synchronize()
    for t in (y_h, y_f, g, ly):
        assert not bool(t.any()), "a refused call wrote its output"
    # the same calls with the argument put right are accepted
    L.check(lib.hm_sar_graph_mix(L.ptr(lap_h), 800, L.ptr(x_h), 16, L.ptr(y_h), s))
    L.check(lib.hm_sar_linear_f32(L.ptr(lx), 4, 64, L.ptr(lw), L.ptr(bias), L.ptr(ly), 8, 0, s))
    torch.cuda.synchronize()
