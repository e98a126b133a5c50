"""Host check of the exact-integer test data (tests/exact_data.py): does it tell one operand index from another?

For every shape the strict GPU tests run, the operands are built and the torch reference computed; then each fault of a
catalogue -- the index mistakes a tiled, ring-buffered, lane-mapped kernel can make -- is applied to ONE operand of the
REFERENCE and the reference recomputed.  A fault must change more than half of the outputs: data under which it changes
none (operands constant or periodic along the axis) lets a kernel with that very mistake pass torch.equal.  Nothing here
imports, runs or emulates the compiled library; the catalogue acts on reference operands only.

Large problems are checked on a 256 x 256 subset of the output spread evenly over the rows and columns (so over every tile);
a fault is an index map, applied to the full operand's indices before the subset is taken.  A fault that is the identity
map at a shape (a rotation of K-tiles when K is one tile, a flip of a 1 x 1 kernel) is no fault there and is passed over;
each list must still meet every fault of its catalogue at some shape.
"""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exact_data as ED  # noqa: E402

SUB = 256
HALF = 0.5


def _spread(n, k=SUB):
    k = min(n, k)
    return (torch.arange(k, dtype=torch.int64) * n) // k


def _ar(n):
    return torch.arange(n, dtype=torch.int64)


# ------------------------------------------------------------------------------------------------ index maps
def k_tiles_rotated(K):
    k = _ar(K)
    return ((k // 64 + 1) % (K // 64)) * 64 + k % 64


def k_chunks_swapped(K):                       # neighbouring 8-wide chunks of a K-tile change places
    k = _ar(K)
    return (k // 8 ^ 1) * 8 + k % 8


def k_lanes_swapped(K):                        # the four k of a lane group in reverse
    return _ar(K) ^ 3


def k_tail_is_first_tile(K):                   # the last K-tile read from the first one's slot
    k = _ar(K)
    return torch.where(k >= K - 64, k % 64, k)


def k_upper_half_from_previous_tile(K):        # k 32..63 of every tile from the tile before (the first from the last)
    k = _ar(K)
    return torch.where(k % 64 >= 32, (k - 64) % K, k)


def k_tiles_0_1_swapped(K):
    k = _ar(K)
    return torch.where(k < 64, k + 64, torch.where(k < 128, k - 64, k)) if K >= 128 else k


def rotated(by):
    return lambda n: (_ar(n) + by) % n


def flipped(n):
    return _ar(n).flip(0)


def _is_identity(m):
    return torch.equal(m, _ar(m.numel()))


# (name, operand, axis, map): operand in x / w / bias / resid (+ xs / ws for fp8), axis 0 = rows, 1 = K (columns of x and w)
GEMM_FAULTS = [
    ("W: 64-wide K-tiles rotated by one", "w", 1, k_tiles_rotated),
    ("W: 8-wide chunks swapped inside a K-tile", "w", 1, k_chunks_swapped),
    ("W: k-lanes swapped inside groups of 4", "w", 1, k_lanes_swapped),
    ("W: last K-tile replaced by the first", "w", 1, k_tail_is_first_tile),
    ("W: upper 32 k of a tile from the previous tile", "w", 1, k_upper_half_from_previous_tile),
    ("X: K-tiles 0 and 1 swapped", "x", 1, k_tiles_0_1_swapped),
    ("X: 8-wide chunks swapped inside a K-tile", "x", 1, k_chunks_swapped),
    ("W rows rotated by 80", "w", 0, rotated(80)),
    ("W rows rotated by 16", "w", 0, rotated(16)),
    ("X rows rotated by 16", "x", 0, rotated(16)),
    ("X rows rotated by 128", "x", 0, rotated(128)),
    ("bias rotated by 16", "bias", 0, rotated(16)),
    ("bias rotated by 1", "bias", 0, rotated(1)),
    ("residual rows rotated by 16", "resid", 0, rotated(16)),
    ("residual rows rotated by resid_mod (192)", "resid", 0, rotated(192)),
    ("residual columns rotated by 64", "resid", 1, rotated(64)),
]
FP8_FAULTS = [f for f in GEMM_FAULTS if f[1] in ("x", "w")] + [
    ("X: 32-wide scale blocks rotated against the data", "xs", 0, rotated(1)),
    ("X: scale columns (rows of X) rotated by 16", "xs", 1, rotated(16)),
    ("W: row scales rotated by 16", "ws", 0, rotated(16)),
]
# operand, axis of the NCHW / (Co, Ci, kh, kw) tensor
CONV_FAULTS = [
    ("conv W: ci rotated by 8", "w", 1, rotated(8)),
    ("conv W: ci rotated by 3", "w", 1, rotated(3)),
    ("conv W: kh flipped", "w", 2, flipped),
    ("conv W: kw flipped", "w", 3, flipped),
    ("conv X: ci rotated by 8", "x", 1, rotated(8)),
    ("conv X: ci rotated by 5", "x", 1, rotated(5)),
    ("conv W: output channels rotated by 8 against the bias", "w", 0, rotated(8)),
    ("conv bias rotated by 8", "bias", 0, rotated(8)),
]


# ------------------------------------------------------------------------------------------------ GEMM
def _gemm_sub(ops, rows, cols, maps=None):
    """(x @ w^T + bias + resid[m % resid_rows]) on the output subset rows x cols, operand indices sent through `maps`."""
    maps = maps or {}

    def ix(op, axis, idx):
        m = maps.get((op, axis))
        return idx if m is None else m[idx]

    x, w, bias, resid = ops["x"], ops["w"], ops.get("bias"), ops.get("resid")
    K = x.shape[1]
    xs = x[ix("x", 0, rows)][:, ix("x", 1, _ar(K))]
    ws = w[ix("w", 0, cols)][:, ix("w", 1, _ar(K))]
    y = xs @ ws.t()
    if bias is not None:
        y = y + bias[ix("bias", 0, cols)]
    if resid is not None:
        y = y + resid[ix("resid", 0, rows % resid.shape[0])][:, ix("resid", 1, cols)]
    return y


def _run_catalogue(faults, ops, compute, sizes):
    """Fractions of outputs each applicable fault changes; `sizes[(operand, axis)]` is the length of that axis."""
    ref = compute(None)
    seen, low = set(), []
    for name, op, axis, fn in faults:
        if ops.get(op) is None:
            continue
        m = fn(sizes[(op, axis)])
        if _is_identity(m):
            continue
        frac = float((compute({(op, axis): m}) != ref).float().mean())
        seen.add(name)
        if not frac > HALF:
            low.append((name, round(frac, 4)))
    return ref, seen, low


def _gemm_catalogue(M, N, K, bias=True, resid=None, resid_rows=None):
    x, w, b, r = ED.gemm_case(M, N, K, bias=bias, resid=resid, resid_rows=resid_rows)
    assert ED.exact_bound(x, w, K, b, r) < ED.EXACT_LIMIT
    ops = {"x": x, "w": w, "bias": b, "resid": r}
    rows, cols = _spread(M), _spread(N)
    sizes = {("x", 0): M, ("x", 1): K, ("w", 0): N, ("w", 1): K, ("bias", 0): N}
    if r is not None:
        sizes[("resid", 0)], sizes[("resid", 1)] = r.shape
    ref, seen, low = _run_catalogue(GEMM_FAULTS, ops, lambda maps: _gemm_sub(ops, rows, cols, maps), sizes)
    assert not low, ((M, N, K), low)
    assert float(ref.abs().max()) < ED.EXACT_LIMIT
    return ref, seen, ops


def _rounds_in_bf16(ref):
    return bool((ref.to(torch.bfloat16).float() != ref).any())


# (list name, shapes as (M, N, K), bias, resid range, bf16 store path exercised)
GEMM_LISTS = [
    ("asymmetric", ED.GEMM_ASYMMETRIC, False, None, False),
    ("tile_variants", ED.GEMM_TILE_VARIANTS, True, None, False),
    ("deep_prefetch", ED.GEMM_DEEP_PREFETCH, True, 5, True),
    ("persistent", ED.GEMM_PERSISTENT, True, None, True),
    ("persistent_fallback", ED.GEMM_PERSISTENT_FALLBACK, False, None, False),
    ("inloop_residual", ED.GEMM_INLOOP_RESIDUAL, True, ED.GEMM_INLOOP_RESIDUAL_RANGE, False),
    ("strided", ED.GEMM_STRIDED, True, 5, True),
    ("f32", ED.gemm_f32_shapes(), True, 5, False),
    ("f32_strided", ED.GEMM_F32_STRIDED, True, 5, False),
]


@pytest.mark.parametrize("name,shapes,bias,resid,bf16", GEMM_LISTS, ids=[g[0] for g in GEMM_LISTS])
def test_gemm_data_sees_every_fault(name, shapes, bias, resid, bf16):
    """Every GEMM fault changes more than half of the outputs at every shape of the list; the exactness bound holds; where the
    list's test stores bf16, the expected output holds integers bf16 cannot represent (|v| > 256, odd) at every shape with
    K >= 1280, so the store path's round-to-nearest-even is exercised on exact inputs."""
    met, rounded = set(), False
    for (M, N, K) in shapes:
        ref, seen, ops = _gemm_catalogue(M, N, K, bias=bias, resid=resid)
        met |= seen
        if bf16:
            store = _gemm_sub({"x": ops["x"], "w": ops["w"], "bias": ops["bias"]}, _spread(M), _spread(N))
            if K >= 1280:
                assert _rounds_in_bf16(store), (M, N, K)
            rounded |= _rounds_in_bf16(store)
    expect = {f[0] for f in GEMM_FAULTS if (f[1] != "bias" or bias) and (f[1] != "resid" or resid)}
    if all(192 % M == 0 for (M, _, _) in shapes):          # a rotation by 192 is the identity on 192 rows (and on one)
        expect -= {"residual rows rotated by resid_mod (192)"}
    assert met == expect, expect - met
    assert rounded or not bf16


def test_gemm_tile_rule_data_sees_every_fault():
    """The 7 x 3 shapes of test_gemm_tile_rule_exact_at_every_batch_size (M = hands * 192), with the residual where the test has one."""
    for (M, N, K, epi) in ED.gemm_tile_rule_shapes():
        _gemm_catalogue(M, N, K, bias=True, resid=5 if epi == "resid" else None)


def test_gemm_f32_positional_residual_sees_every_fault():
    """resid_mod = 192: a (192, N) residual added to row m % 192, as patch_embed adds the positional embedding."""
    for (M, N, K) in ED.gemm_f32_shapes() + ED.GEMM_F32_STRIDED:
        if M % 192 == 0:
            _gemm_catalogue(M, N, K, bias=True, resid=5, resid_rows=192)


# ------------------------------------------------------------------------------------------------ fp8
def test_fp8_data_sees_every_fault():
    for (M, N, K) in ED.GEMM_FP8:
        x8, xs, w8, ws, xi, wi = ED.fp8_case(M, N, K)
        ops = {"x": xi, "w": wi, "xs": xs, "ws": ws}
        sizes = {("x", 0): M, ("x", 1): K, ("w", 0): N, ("w", 1): K, ("xs", 0): K // 32, ("xs", 1): M, ("ws", 0): N}

        def compute(maps):
            o = dict(ops)
            for (op, axis), m in (maps or {}).items():
                o[op] = o[op].index_select(axis, m)
            return ED.fp8_reference(o["x"], o["xs"], o["w"], o["ws"])

        ref, seen, low = _run_catalogue(FP8_FAULTS, ops, compute, sizes)
        assert not low, low
        assert seen == {f[0] for f in FP8_FAULTS}
        # exact in fp32: the fp64 reference survives the round trip, and so does the unit of the smallest scales
        assert torch.equal(ref.float().double(), ref)
        assert float(ref.abs().max()) / (2.0 ** -1 * 2.0 ** -1) < ED.EXACT_LIMIT
        # the bytes the kernel takes are the integers the reference used
        assert torch.equal(x8.view(torch.float8_e4m3fn).float(), xi) and torch.equal(w8.view(torch.float8_e4m3fn).float(), wi)
        assert int(xs.min()) == 126 and int(xs.max()) == 129 and sorted(set(ws.tolist())) == [0.5, 1.0, 2.0]


# ------------------------------------------------------------------------------------------------ convolution
CONV_LISTS = [("basic", ED.CONV_BASIC), ("every_tile", ED.CONV_EVERY_TILE), ("k_groups", ED.CONV_K_GROUPS),
              ("lean_loader", ED.CONV_LEAN_LOADER), ("serial_k", ED.CONV_SERIAL_K), ("split_k", ED.CONV_SPLIT_K), ("f32", ED.CONV_F32)]


@pytest.mark.parametrize("name,shapes", CONV_LISTS, ids=[c[0] for c in CONV_LISTS])
def test_conv_data_sees_every_fault(name, shapes):
    """Every convolution fault changes more than half of the outputs at every shape of the list (on the first two images of
    the large batches: conv_case's data does not depend on the batch size, and no fault acts along the batch)."""
    met = set()
    for (n, Ci, Co, k, s, H, W) in shapes:
        x, w, b = ED.conv_case(min(n, 2), Ci, Co, k, H, W)
        assert ED.exact_bound(x, w, Ci * k * k, b) < ED.EXACT_LIMIT
        if n > 2:
            assert torch.equal(ED.conv_case(3, Ci, Co, k, H, W)[0][:2], x)
        ops = {"x": x, "w": w, "bias": b}
        sizes = {(op, ax): ops[op].shape[ax] for op in ops for ax in range(ops[op].dim())}

        def compute(maps):
            o = dict(ops)
            for (op, axis), m in (maps or {}).items():
                o[op] = o[op].index_select(axis, m)
            return F.conv2d(o["x"], o["w"], o["bias"], stride=s, padding=k // 2)

        ref, seen, low = _run_catalogue(CONV_FAULTS, ops, compute, sizes)
        assert not low, ((Ci, Co, k, s, H, W), low)
        met |= seen
    expect = {f[0] for f in CONV_FAULTS}
    if all(k == 1 for (_, _, _, k, _, _, _) in shapes):
        expect -= {"conv W: kh flipped", "conv W: kw flipped"}
    assert met == expect, expect - met


# ------------------------------------------------------------------------------------------------ the data and the report
def test_ints_are_hashed_integers_in_range_without_a_period():
    t = ED.ints("t", (64, 640), -3, 3, seed=1)
    assert t.dtype == torch.float32 and torch.equal(t, t.round()) and float(t.min()) == -3 and float(t.max()) == 3
    assert torch.equal(t, ED.ints("t", (64, 640), -3, 3, seed=1))                                  # a pure function of (tag, seed, index)
    assert torch.equal(t.reshape(-1), ED.ints("t", (64 * 640,), -3, 3, seed=1, chunk=1000))        # whatever the chunking
    assert not torch.equal(t, ED.ints("t", (64, 640), -3, 3, seed=2)) and not torch.equal(t, ED.ints("u", (64, 640), -3, 3, seed=1))
    for shift in (1, 2, 3, 4, 5, 7, 8, 16, 32, 64, 128, 640):                                       # no period along either axis
        flat = t.reshape(-1)
        assert 0.8 < float((flat[shift:] != flat[:-shift]).float().mean()) < 0.9, shift              # 6/7 for independent values
    counts = torch.bincount((t + 3).long().reshape(-1), minlength=7).float() / t.numel()
    assert float((counts - 1 / 7).abs().max()) < 0.01


def test_builders_refuse_data_that_is_not_exact(monkeypatch):
    monkeypatch.setattr(ED, "EXACT_LIMIT", 1000.0)
    with pytest.raises(AssertionError):
        ED.gemm_case(64, 64, 256)
    with pytest.raises(AssertionError):
        ED.conv_case(1, 64, 8, 3, 8, 8)
    with pytest.raises(AssertionError):
        ED.fp8_case(16, 64, 128)


def test_assert_exact_locates_the_fault():
    ref = ED.ints("r", (300, 200), -9, 9)
    ED.assert_exact(ref.clone(), ref, "same")
    got = ref.clone()
    got[130:140, 64:128] += 1.0
    with pytest.raises(AssertionError) as e:
        ED.assert_exact(got, ref, "case (300, 200)")
    msg = str(e.value)
    assert "case (300, 200)" in msg and "640 of 60000 elements wrong" in msg and "first at (row 130, col 64)" in msg
    assert f"got {got[130, 64].item()!r}, expected {ref[130, 64].item()!r}" in msg
    assert "64-row blocks with errors 1 of 5: [2]" in msg and "64-column blocks with errors 1 of 4: [1]" in msg
    with pytest.raises(AssertionError, match="shape"):
        ED.assert_exact(ref[:, :10], ref, "shape")
    with pytest.raises(AssertionError, match="dtype"):
        ED.assert_exact(ref.half(), ref, "dtype")
    nan = ref.clone()
    nan[5, 7] = float("nan")
    with pytest.raises(AssertionError, match=r"first at \(row 5, col 7\)"):
        ED.assert_exact(nan, ref, "nan")
    # NCHW results are located as the implicit GEMM's (pixel row, channel column)
    r4 = ED.ints("r4", (2, 8, 5, 6), -9, 9)
    g4 = r4.clone()
    g4[1, 3, 2, 4] += 1.0
    with pytest.raises(AssertionError, match=r"1 of 480 elements wrong; first at \(row 46, col 3\)"):
        ED.assert_exact(g4, r4, "conv")
