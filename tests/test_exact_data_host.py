"""Host check of the exact-integer test data (tests/exact_data.py): does it tell one operand index from another?

For every shape the strict GPU tests run, the operands are built and the torch reference computed; then each fault of a
catalogue -- the index mistakes a tiled, ring-buffered, lane-mapped kernel can make -- is applied to ONE operand of the
REFERENCE and the reference recomputed.  A fault must change more than half of the outputs: data under which it changes
none (operands constant or periodic along the axis) lets a kernel with that very mistake pass torch.equal.  Nothing here
imports, runs or emulates the compiled library; the catalogue acts on reference operands only.

The LayerNorm data (ED.ln_case, ED.ln_accum_case) has a catalogue of its own: rows, columns, 256-column pieces and lane pairs
of the row kernels, slabs and bias of the accumulating one, layout and neighbours of the MXFP8 scales.  Its row dependence is
one sign per element, so a fault changes about half of what it moves: the bar is 40 % of the values and 20 % of the scale bytes.
The error bound of the GPU accuracy test is measured and checked against wrong formulas here as well.

The SAR hand-mesh head (section "SAR hand-mesh head") gets the GEMM catalogue at its own shapes plus the faults its kernels
alone can make (the 32-wide K loop, the transposed read's halves, the SAIGB scatter), and catalogues of their own for the
few-hot soft-argmax data and the dyadic post-processing data; the fp32 rule of tests/sar_rule.py must reproduce both closed forms.

The MANO tail, the Detect decode and the RootNet layout kernels (the last sections) have rules that take a `fault` argument:
each fault of their catalogues is applied to the rule at every case the GPU tests run and must change more than half of the
rows of the output it concerns; the decode's closeness bound is measured here, on the CPU, against float64.

The fp8 epilogue data (ED.fp8_epilogue_case) meets FP8_FAULTS at every shape of both fp8 kernels, judged on its three expectations
(fp32, bf16, GELU -> MXFP8 bytes and scales); the attention data (ED.attention_case) has a rule with a `fault` argument
(tests/attention_rule.py) and the scale faults of the LayerNorm -> MXFP8 data for its MXFP8 form.

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
import tome_rule as TR  # noqa: E402

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
    return ((k // 64 + 1) % (K // 64)) * 64 + k % 64 if K >= 64 else k        # (K % 64 != 0: the partial last tile takes tile 1's slot)


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


# ------------------------------------------------------------------------------------------------ hm_linear_f32
def k_lane_group_transposed(K):                # k-slot g of MFMA i reads k = kb + 4i + g instead of kb + 4g + i
    k = _ar(K)
    return k // 16 * 16 + (k % 4) * 4 + (k % 16) // 4


LINEAR_FAULTS = GEMM_FAULTS + [
    ("X: the four k of a lane group permuted (4i + g)", "x", 1, k_lane_group_transposed),
    ("W: the four k of a lane group permuted (4i + g)", "w", 1, k_lane_group_transposed),
]
LINEAR_WAVES = 4


def linear_wave_not_applicable(shapes):
    """(shape, wave) where the wave has no 16-wide K block: K <= 16 * wave."""
    return {((M, N, K), w) for (M, N, K) in shapes for w in range(LINEAR_WAVES) if K <= 16 * w}


def linear_fault_fractions(shapes):
    """{fault name: [(fraction of outputs changed, shape), ...]} over the index-map catalogue and the four dropped waves, and
    the set of (shape, wave) at which a dropped wave is no fault because the wave has no K block."""
    table, na = {}, set()
    for (M, N, K) in shapes:
        x, w, b, r = ED.gemm_case(M, N, K, resid=5)
        assert ED.exact_bound(x, w, K, b, r) < ED.EXACT_LIMIT
        ops = {"x": x, "w": w, "bias": b, "resid": r}
        rows, cols = _spread(M), _spread(N)
        sizes = {("x", 0): M, ("x", 1): K, ("w", 0): N, ("w", 1): K, ("bias", 0): N, ("resid", 0): M, ("resid", 1): N}
        ref = _gemm_sub(ops, rows, cols)
        assert float(ref.abs().max()) < ED.EXACT_LIMIT
        for name, op, axis, fn in LINEAR_FAULTS:
            m = fn(sizes[(op, axis)])
            if _is_identity(m):
                continue
            frac = float((_gemm_sub(ops, rows, cols, {(op, axis): m}) != ref).float().mean())
            table.setdefault(name, []).append((frac, (M, N, K)))
        for wave in range(LINEAR_WAVES):
            name = f"wave {wave}'s 16-wide K blocks dropped"
            mine = (_ar(K) // 16) % LINEAR_WAVES == wave
            if not bool(mine.any()):
                na.add(((M, N, K), wave))
                continue
            xz = x.clone()
            xz[:, mine] = 0.0
            frac = float((_gemm_sub(dict(ops, x=xz), rows, cols) != ref).float().mean())
            table.setdefault(name, []).append((frac, (M, N, K)))
    return table, na


@pytest.mark.parametrize("name,shapes", [("prod", ED.LINEAR_F32_PROD), ("edge", ED.LINEAR_F32_EDGE)])
def test_linear_f32_data_sees_every_fault(name, shapes):
    """The GEMM catalogue, the lane map k = kb + 4i + g on either operand and each of the four waves' K blocks dropped change
    more than half of the outputs at every hm_linear_f32 shape.  A dropped wave is no fault where the wave has no block
    (K = 16: waves 1-3, K = 48: wave 3): those are listed, and the list is exactly that.  Smallest fractions measured: 0.75
    (three of the four outputs of (1, 4, 16)) for the chunk and lane-group faults, 0.75 for the bias rotated by 1 at (1, 20, 64),
    0.875 for a dropped wave (wave 1 at (16, 4, 48)); at the production shapes 0.86 (bias) and 0.98 and more (every K fault)."""
    table, na = linear_fault_fractions(shapes)
    low = [(n, f, sh) for n, rows in table.items() for (f, sh) in rows if not f > HALF]
    assert not low, low
    assert set(table) == {f[0] for f in LINEAR_FAULTS} | {f"wave {w}'s 16-wide K blocks dropped" for w in range(LINEAR_WAVES)}
    assert na == linear_wave_not_applicable(shapes)
    if name == "edge":
        assert {K for (_, K), _ in ((sh[1:], w) for sh, w in na)} == {16, 48} and len({w for _, w in na}) == 3
    else:
        assert not na


def test_linear_f32_edge_shapes_cover_every_value():
    for axis, values in enumerate((ED.LINEAR_F32_M, ED.LINEAR_F32_N, ED.LINEAR_F32_K)):
        for v in values:
            assert sum(sh[axis] == v for sh in ED.LINEAR_F32_EDGE) >= 2, (axis, v)
        assert {sh[axis] for sh in ED.LINEAR_F32_EDGE} == set(values)
    assert len(set(ED.LINEAR_F32_EDGE)) == len(ED.LINEAR_F32_EDGE) and all(sh in ED.LINEAR_F32_PROD + ED.LINEAR_F32_EDGE for sh in ED.LINEAR_F32_STRIDED)
    cfg = ED.synth.HamerConfig()
    assert (64, cfg.dec.dim, cfg.dec.mlp_dim) in ED.LINEAR_F32_PROD and (1, 112, cfg.dec.dim) in ED.LINEAR_F32_PROD
    assert (384, 80, 1280) in ED.LINEAR_F32_PROD and len(ED.LINEAR_F32_PROD) == 13


# ------------------------------------------------------------------------------------------------ token merging
def _tome_metric(T):
    return ED.tome_match_case(ED.TOME_B, T, ED.TOME_SALT.get(T, 0))


def _match_variant(metric, r, last_max=False, high_a_first=False, swapped=False, normalise=True):
    """The matching again, vectorised and in float64, with one decision of the rule changed."""
    m = metric.double()
    if normalise:
        m = m / (m * m).sum(-1, keepdim=True).sqrt()
    a, b = (m[:, 1::2], m[:, 0::2]) if swapped else (m[:, 0::2], m[:, 1::2])
    s = a @ b.transpose(1, 2)
    mx = s.max(-1).values
    j = _ar(s.shape[2])
    at_max = s == mx[..., None]
    best = torch.where(at_max, j, -1).max(-1).values if last_max else torch.where(at_max, j, s.shape[2]).min(-1).values
    unm, src, dst = [], [], []
    for c in range(s.shape[0]):
        p = mx[c].tolist()
        order = sorted(range(len(p)), key=lambda i: (-p[i], -i if high_a_first else i))
        unm.append(order[r:])
        src.append(order[:r])
        dst.append(best[c][order[:r]].tolist())
    B = s.shape[0]
    return tuple(torch.tensor(t, dtype=torch.int64).reshape(B, -1) for t in (unm, src, dst))


def _merge_variant(x, size, unm, src, dst, first_only=False, unweighted=False, size_kept=False):
    """The merge again, with index_add_, and one step of it changed."""
    B, T, D = x.shape
    sz = (torch.ones(B, T) if size is None else size).double()
    xs, ss = [], []
    for b in range(B):
        s_, d_ = src[b], dst[b]
        if first_only:
            keep = [k for k, j in enumerate(d_.tolist()) if j not in d_[:k].tolist()]
            s_, d_ = s_[keep], d_[keep]
        w = torch.ones_like(sz[b]) if unweighted else sz[b]
        xw = x[b].double() * w[:, None]
        num = torch.cat([x[b, 2 * unm[b]].double() * sz[b, 2 * unm[b], None], xw[1::2].index_add(0, d_, xw[2 * s_])])
        den = torch.cat([sz[b, 2 * unm[b]], sz[b, 1::2].index_add(0, d_, sz[b, 2 * s_])])
        xs.append(num.float() / den.float()[:, None])
        ss.append((torch.cat([sz[b, 2 * unm[b]], sz[b, 1::2]]) if size_kept else den).float())
    return torch.stack(xs), torch.stack(ss)


def _same(got, ref):
    return all(g.shape == r.shape and torch.equal(g, r) for g, r in zip(got, ref))


def _changed_fraction(got, ref):
    if any(g.shape != r.shape for g, r in zip(got, ref)):
        return 1.0
    n = sum(r.numel() for r in ref)
    return sum(int((g != r).sum()) for g, r in zip(got, ref)) / max(n, 1)


def _tome_merge_inputs(T, D):
    return ED.tome_merge_case(ED.TOME_B, T, D, ED.tome_sizes_given(T))


def test_tome_rule_is_the_oracle_on_exact_and_random_data():
    """tests/tome_rule.py against oracle.tome_ref.bipartite_match / merge_tokens: indices, merged rows and sizes equal on every
    TOME_EXACT case (where the rule asserts that all its intermediates are exact) and D; on the random-data cases of
    test_tome_kernels_vs_oracle the indices and sizes equal and the merged rows, whose fp32 sums the oracle rounds, within
    that test's own atol = 2e-6, rtol = 1e-6.  The vectorised second statement used for the fault catalogue agrees too."""
    from oracle import tome_ref as T
    for (tokens, r) in ED.TOME_EXACT:
        metric = _tome_metric(tokens)
        mine = TR.match(metric, r)
        assert _same(mine, T.bipartite_match(metric, r)) and _same(mine, _match_variant(metric, r)), (tokens, r)
        assert mine[0].shape == (ED.TOME_B, (tokens + 1) // 2 - r)
        for D in ED.TOME_D:
            x, size = _tome_merge_inputs(tokens, D)
            sz = size if size is not None else torch.ones(ED.TOME_B, tokens)
            xo, so = TR.merge(x, size, *mine)
            x_ref, s_ref = T.merge_tokens(x, sz[..., None], *mine)
            assert torch.equal(xo, x_ref) and torch.equal(so, s_ref[..., 0]), (tokens, r, D)
            assert _same((xo, so), _merge_variant(x, size, *mine))
            assert bool(TR.quotient_representable(x, size, *mine)[:, :mine[0].shape[1]].all())
    B, H, d, D = 3, 4, 80, 320
    for tokens, r, with_size in ((192, 16, False), (161, 14, True), (176, 15, True), (23, 8, True), (17, 4, True), (16, 4, True), (3, 1, True)):
        qkv = ED.synth.uniform("tq", (B * tokens, 3 * H * d), 1.2, seed=tokens).half()
        size = (1.0 + (ED.synth._hash_u32(torch.arange(B * tokens, dtype=torch.int64), 7) % 4).float()).reshape(B, tokens) if with_size else None
        x = ED.synth.uniform("tx", (B * tokens, D), 1.0, seed=tokens + 1).reshape(B, tokens, D)
        metric = qkv.float().reshape(B, tokens, 3, H, d)[:, :, 1].mean(2)
        mine = TR.match(metric, r, exact=False)
        assert _same(mine, T.bipartite_match(metric, r)), (tokens, r)
        xo, so = TR.merge(x, size, *mine, exact=False)
        x_ref, s_ref = T.merge_tokens(x, (size if with_size else torch.ones(B, tokens))[..., None], *mine)
        assert torch.equal(so, s_ref[..., 0])
        torch.testing.assert_close(xo, x_ref, atol=2e-6, rtol=1e-6)
    with pytest.raises(AssertionError):
        TR.match(metric, r)                                 # random data is not exact, and the rule says so


def tome_data_conditions(T, r, metric):
    """What the matching data must contain for the GPU test to decide the tie rules (names of the conditions that fail)."""
    Na = (T + 1) // 2
    unm, src, dst = TR.match(metric, r)
    fails, boundary_tie = [], False
    for c in range(metric.shape[0]):
        s = TR.scores(metric[c])
        p = s.max(1).values
        if len(set(p.tolist())) < 4:
            fails.append(f"crop {c}: fewer than 4 distinct proposal scores")
        norm = (metric[c].double() ** 2).sum(1).sqrt()
        if float(norm.max() / norm.min()) < 4:
            fails.append(f"crop {c}: norms within a factor of 4")
        ranked = sorted(p.tolist(), reverse=True)
        boundary_tie |= r < Na and ranked[r - 1] == ranked[r]
    tied = [(TR.scores(metric[c])[a] == TR.scores(metric[c])[a].max()).sum() >= 2 for c in range(metric.shape[0]) for a in src[c].tolist()]
    if not any(bool(t) for t in tied):
        fails.append("no merged A token whose maximal score is reached by two B tokens")
    if r >= 3:
        counts = torch.stack([torch.bincount(dst[c], minlength=T // 2) for c in range(metric.shape[0])])
        if int(counts.max()) < 3 or int(counts.min()) > 0:
            fails.append("no B token with three merges, or none without one")
    if r < Na and not boundary_tie:
        fails.append("no crop with equal scores at ranks r - 1 and r")
    if _same(_match_variant(metric, r, normalise=False), (unm, src, dst)):
        fails.append("the matching is the same without normalisation")
    return fails


def test_tome_match_data_decides_the_tie_rules():
    """At every TOME_EXACT case with T >= 17: at least 4 distinct proposal scores and norms a factor of 4 apart in every crop; a
    MERGED A token whose maximum is reached by two or more B tokens (so first-versus-last maximum changes a dst); where r >= 3
    (a B token cannot receive three merges otherwise) a B token with three or more merges and one with none; where r < Na,
    equal scores at ranks r - 1 and r in some crop (the tie rule decides WHO is merged); another matching without
    normalisation.  The data is integer-valued, hashed per crop, and a pure function of (B, T, salt)."""
    for (T, r) in ED.TOME_EXACT:
        metric = _tome_metric(T)
        assert torch.equal(metric, _tome_metric(T)) and not torch.equal(metric[0], metric[1]) and not torch.equal(metric[1], metric[2])
        mags = metric.abs().amax(-1)
        assert set(mags.unique().tolist()) <= set(map(float, ED.TOME_MAGNITUDES)) and bool(((metric == 0) | (metric.abs() == mags[..., None])).all())
        assert set((metric != 0).sum(-1).unique().tolist()) <= set(ED.TOME_SUPPORTS)
        for kind in ED.TOME_LAYOUTS:                                             # the layouts hold the metric, and something else around it
            buf, first, cols, lo_off = ED.tome_metric_layout(metric, kind)
            view = buf[:, first:first + cols]
            value = view[:, :80] + (view[:, lo_off:lo_off + 80] if lo_off else 0)
            assert torch.equal(value.reshape(ED.TOME_B, T, 80), metric) and buf.shape[1] == {"ld80": 80, "ld96": 96, "hi_lo": 176}[kind]
            outside = torch.ones_like(buf, dtype=torch.bool)
            outside[:, first:first + 80] = False
            if lo_off:
                outside[:, first + lo_off:first + lo_off + 80] = False
                assert not torch.equal(view[:, :80].reshape(ED.TOME_B, T, 80), metric)
            assert bool((buf[outside] == ED.TOME_FILL).all())
        for dt in (torch.float16, torch.bfloat16):                               # (the builder asserts the head mean and the 16-bit exactness)
            assert ED.tome_head_keys(metric, 4, dt).shape == (ED.TOME_B * T, 3 * 4 * 80)
        if T >= 17:
            assert bool((metric != 0).any(0).any(0).all())                       # every channel is used
            fails = tome_data_conditions(T, r, metric)
            assert not fails, ((T, r), fails)


def tome_rule_fault_table():
    """{fault: [(fraction of indices and merged values changed, (T, r)), ...]} and {fault: [(T, r) it does not apply to]}.
    Matching faults are judged on (unm, src, dst) and the rows merged with them, merge faults on (x_out, size_out)."""
    table, na = {}, {}

    def note(name, applies, case, got, ref):
        if applies:
            table.setdefault(name, []).append((_changed_fraction(got, ref), case))
        else:
            na.setdefault(name, []).append(case)

    for (T, r) in ED.TOME_EXACT:
        metric = _tome_metric(T)
        ref = TR.match(metric, r)
        x, size = _tome_merge_inputs(T, ED.TOME_D[0])
        out = TR.merge(x, size, *ref)
        big = T >= 17                      # below, the crops hold one to four A tokens: ties and crowded B tokens are not promised
        B = ED.TOME_B

        def matched(name, applies, got):
            full = got + _merge_variant(x, size, *got) if all(g.shape == f.shape for g, f in zip(got, ref)) else got
            note(name, applies, (T, r), full, ref + out)

        matched("last maximum instead of the first", big, _match_variant(metric, r, last_max=True))
        matched("equal scores ranked higher a first", big, _match_variant(metric, r, high_a_first=True))
        matched("A and B sets swapped", T >= 3, _match_variant(metric, r, swapped=True))
        matched("no normalisation", big, _match_variant(metric, r, normalise=False))
        buf, first, cols, lo_off = ED.tome_metric_layout(metric, "hi_lo")
        matched("lo part ignored", big, _match_variant(buf[:, first:first + 80].reshape(B, T, 80), r))
        buf, first, cols, lo_off = ED.tome_metric_layout(metric, "ld96")
        matched("metric read with row stride 80 in the ld = 96 layout", big, _match_variant(buf.reshape(-1)[first:first + B * T * 80].reshape(B, T, 80), r))
        matched("crop 0's indices used for every crop", big, tuple(t[:1].expand(B, -1) for t in ref))
        crowded = big and r >= 3
        note("only the first proposer merged into a dst", crowded, (T, r), _merge_variant(x, size, *ref, first_only=True), out)
        note("size weights ignored in the sum", size is not None, (T, r), _merge_variant(x, size, *ref, unweighted=True), out)
        note("size not accumulated into size_out", True, (T, r), _merge_variant(x, size, *ref, size_kept=True), out)
    return table, na


def test_tome_rule_fault_catalogue():
    """Each wrong rule changes the indices or the merged rows at every case it applies to.  Not applicable, and listed: the
    tie, normalisation, layout and crop faults below T = 17 (a crop of 2 or 3 tokens has one B token and promises no tie);
    swapped sets at T = 2 (either way the two tokens end as one); a crowded B token where r < 3; size weights where no sizes
    are given (T = 192)."""
    table, na = tome_rule_fault_table()
    low = [(n, f, c) for n, rows in table.items() for (f, c) in rows if not f > 0]
    assert not low, low
    assert len(table) == 10 and all(len(table[n]) + len(na.get(n, [])) == len(ED.TOME_EXACT) for n in table)
    small = [(3, 1), (2, 1)]
    assert na == {
        "last maximum instead of the first": small, "equal scores ranked higher a first": small, "no normalisation": small,
        "lo part ignored": small, "metric read with row stride 80 in the ld = 96 layout": small,
        "crop 0's indices used for every crop": small, "A and B sets swapped": [(2, 1)],
        "only the first proposer merged into a dst": [(129, 1)] + small,
        "size weights ignored in the sum": [(192, 16), (192, 96)],
    }


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
    met = set()
    for (M, N, K) in FP8_EPILOGUE_SHAPES:
        met |= _fp8_epilogue_catalogue(M, N, K)
    assert met == {f[0] for f in FP8_FAULTS}


FP8_EPILOGUE_SHAPES = sorted(set(ED.GEMM_FP8_ONE_TILE) | {s[:3] for s in ED.GEMM_FP8_PERSISTENT} | set(ED.GEMM_FP8_WIDE) | set(ED.GEMM_FP8_NO_BIAS))


def _mx8_scale_faults(sc):
    """The three scale faults of test_ln_mx8_scales_see_every_fault on scale bytes (blocks, rows): (name, faulty, applies)."""
    nblk, M = sc.shape
    return [("scales written [M][blocks]", sc.t().contiguous().view(nblk, M), nblk > 1 and M > 1),
            ("scale of the neighbouring block", sc.roll(1, 0), nblk > 1),
            ("scale of the neighbouring row", sc.roll(1, 1), M > 1)]


FP8_PARTIAL_K = ("W: last K-tile replaced by the first", "X: K-tiles 0 and 1 swapped")
FP8_PARTIAL_SHARE = 1.0 / 3.0


def _fp8_gelu_bar(name, op, axis, m):
    """The share of the GELU -> MXFP8 bytes in positive-bias columns a fault must change: VALUE_FAULT for every fault of
    FP8_FAULTS -- those that re-pair every product of the K loop included (measured 0.42-0.67 at the listed shapes) -- except
    the two that REPLACE part of K (one 64-wide tile; two tiles exchanged) where that part is under a third of K.  There the
    sum moves by a fraction of its spread, and e4m3's three mantissa bits at 448 2^kb showed it in 0.09-0.35 of the bytes
    (0.09 at K = 5120, one tile of 80); the bar is then the moved share of K itself, which the data meets everywhere with
    room, so the sensitivity cannot vanish unnoticed.  The fp32 and bf16 expectations hold these two to HALF at every shape."""
    if axis == 1 and op in ("x", "w"):
        share = float((m != _ar(m.numel())).float().mean())
        if share < FP8_PARTIAL_SHARE:
            assert name in FP8_PARTIAL_K, name
            return share
    return VALUE_FAULT


def _fp8_epilogue_catalogue(M, N, K):
    """FP8_FAULTS against the three expectations of ED.fp8_epilogue_case: acc + bias + resid in fp32 and acc + bias rounded to
    bf16 (more than HALF of the elements change), the GELU -> MXFP8 bytes in the positive-bias columns (at least _fp8_gelu_bar);
    the three output-scale faults change at least SCALE_FAULT of the scale bytes; all-zero blocks exist where N >= 320."""
    c = ED.fp8_epilogue_case(M, N, K)
    ops = {k: c[k] for k in ("xs", "ws")}
    ops["x"], ops["w"] = c["xi"], c["wi"]
    sizes = {("x", 0): M, ("x", 1): K, ("w", 0): N, ("w", 1): K, ("xs", 0): K // 32, ("xs", 1): M, ("ws", 0): N}
    bias, resid, gb, pos = c["bias"].double(), c["resid"].double(), c["gelu_bias"].double(), c["positive"]
    assert int(pos.sum()) >= N // 4

    def expectations(acc):
        return acc + bias + resid, (acc + bias).float().to(torch.bfloat16), ED.fp8_gelu_expect(acc + gb)[0][:, pos]

    ref = expectations(c["acc"])
    assert torch.equal(ref[0].float().double(), ref[0]) and _rounds_in_bf16((c["acc"] + bias).float())
    seen, low = set(), []
    for name, op, axis, fn in FP8_FAULTS:
        m = fn(sizes[(op, axis)])
        if _is_identity(m):
            continue
        o = dict(ops)
        o[op] = o[op].index_select(axis, m)
        bad = expectations(ED.fp8_reference(o["x"], o["xs"], o["w"], o["ws"]))
        fr = [float((b != r).float().mean()) for b, r in zip(bad, ref)]
        seen.add(name)
        if not (fr[0] > HALF and fr[1] > HALF and fr[2] >= _fp8_gelu_bar(name, op, axis, m)):
            low.append((name, [round(f, 4) for f in fr]))
    assert not low, ((M, N, K), low)
    q, sc = ED.fp8_gelu_expect(c["acc"] + gb)
    assert sc.shape == (N // 32, M)
    for name, bad, applies in _mx8_scale_faults(sc):
        assert applies
        frac = float((bad != sc).float().mean())
        assert frac >= SCALE_FAULT, ((M, N, K), name, frac)
    zero = sc == 0
    assert N < 320 or bool(zero.any()), (M, N, K)
    assert bool((q.reshape(M, N // 32, 32)[zero.t()] & 0x7F == 0).all())                 # a zero-scale block is all zero bytes
    assert max(len(set(r.tolist())) for r in sc) >= 2 and max(len(set(col.tolist())) for col in sc.t()) >= 2
    # the bytes the kernel takes are the integers the reference used
    assert torch.equal(c["x8"].view(torch.float8_e4m3fn).float(), c["xi"]) and torch.equal(c["w8"].view(torch.float8_e4m3fn).float(), c["wi"])
    assert int(c["xs"].min()) == 126 and int(c["xs"].max()) == 129
    assert set(c["ws"].tolist()) <= {0.25, 0.5, 1.0, 2.0, 4.0} and len(set(c["ws"].tolist())) >= 3
    return seen


# ------------------------------------------------------------------------------------------------ attention
ATT_CASES = ([("dense", B, h, ED.ATT_T, gs, None) for (B, h, gs) in ED.ATT_DENSE] + [("f32", B, h, ED.ATT_T, gs, None) for (B, h, gs) in ED.ATT_F32]
             + [("tome", ED.ATT_TOME_B, ED.ATT_TOME_HEADS, T, gs, sz) for T in ED.att_tome_tokens()
                for (gs, sz) in (((1,), None), ((1,), "hashed"), ((1, 2, 4), None))]
             + [("tome", ED.ATT_TOME_B, ED.ATT_TOME_HEADS, ED.ATT_TOME_DECIDES, (3,), "decides")])


def _att_rows(out):
    B, H, T, d = out.shape
    return out.permute(0, 2, 1, 3).reshape(B * T, H * d)


def test_attention_data_is_exact_and_sees_every_fault():
    """At every case the exact attention tests run: the plain float64 rule gives the builder's closed form bit for bit (the
    builder itself asserts the gap of 160 log2 units, that every key is some query's chosen key and that the result is
    exact); each fault of attention_rule.FAULTS changes at least HALF of the output elements of the queries it concerns
    (those with a chosen key whose V row, score or output row the fault moves -- a dropped tile concerns a twelfth of the
    queries and cannot do more); every fault is met at every case with 192 tokens."""
    import attention_rule as AR
    for kind, B, H, T, gs, sz in ATT_CASES:
        c = ED.attention_case(B, H, T, gs, sz)
        assert c["gap"] >= ED.ATT_GAP
        ref = AR.attention_rule(c["q"], c["k"], c["v"], ED.ATT_C, c["log2size"])
        assert torch.equal(_att_rows(ref), c["expect"]), (kind, B, H, T, gs, sz)
        ar = _ar(T)
        met = set()
        for fault in AR.FAULTS:
            vmap = AR.v_key_map(fault, T)
            if fault == "one key tile dropped":
                tile = min(AR.DROPPED_TILE, (T - 1) // 16)
                moved = (ar // 16 == tile)
            elif not _is_identity(vmap) or fault in ("V read without the slot permutation", "V rows of neighbouring 16-key tiles swapped"):
                moved = vmap != ar
            else:
                moved = None
            if moved is not None:                                  # queries that put weight on a moved key
                rows = (c["weights"] * moved.double()).sum(-1) > 0
                # every key is some query's chosen key, so the concerned queries are at least the moved share of the keys
                # in every (crop, head) -- half for the slot permutation, a twelfth for the dropped tile at 192 tokens -- and
                # exactly that share where every group is one key
                share, per_item = float(moved.double().mean()), rows.double().mean(-1)
                assert float(per_item.min()) >= share - 1e-12, ((kind, B, H, T, gs, sz), fault, share)
                assert len(gs) > 1 or gs == (3,) or bool((per_item == moved.double().mean()).all())
                if T == ED.ATT_T:
                    assert share == {"V read without the slot permutation": 0.5, "one key tile dropped": 1.0 / 12}.get(fault, 1.0)
            elif fault.startswith("query rows"):
                rows = ((ar // 16 ^ 1) * 16 + ar % 16 < T).expand(B, H, T)
                if T < 32:
                    continue
                assert int(rows[0, 0].sum()) >= T // 32 * 32                 # every whole pair of query tiles
            else:
                rows = torch.ones(B, H, T, dtype=torch.bool)
            if B * H == 1 or (fault == "head index off by one" and H == 1) or not bool(rows.any()):
                continue
            bad = AR.attention_rule(c["q"], c["k"], c["v"], ED.ATT_C, c["log2size"], fault=fault)
            changed = (bad != ref) | bad.isnan()
            frac = float(changed[rows].float().mean())
            met.add(fault)
            assert frac >= HALF, ((kind, B, H, T, gs, sz), fault, frac)
        if T == ED.ATT_T:
            assert met == set(AR.FAULTS), set(AR.FAULTS) - met
        # every query tile of 16 appears (all T queries run), and key 0 and key T - 1 are chosen keys
        assert all(bool((c["chosen"] == t).any(-1).all()) for t in (0, T - 1))
        if sz == "decides":
            w = sorted(set(c["weights"].unique().tolist()))
            assert w == [0.0, 0.25, 0.5], w
        if len(gs) > 1 and T >= 8:
            assert set(c["weights"].unique().tolist()) >= {0.25, 0.5, 1.0}


def test_attention_mx8_scales_see_every_fault():
    """The MXFP8 form of every dense case: the three scale faults change at least SCALE_FAULT of the expected scale bytes; the
    bytes take at least three values along the rows of some block and two along the blocks of some row; the 16 pad columns
    of every head are zero bytes."""
    for (B, H, gs) in ED.ATT_DENSE:
        c = ED.attention_case(B, H, ED.ATT_T, gs)
        q8, sc = ED.att_mx8_expect(c["expect"], H)
        assert q8.shape == (B * ED.ATT_T, H * ED.ATT_HDP) and sc.shape == (H * 3, B * ED.ATT_T)
        for name, bad, applies in _mx8_scale_faults(sc):
            assert applies
            frac = float((bad != sc).float().mean())
            assert frac >= SCALE_FAULT, ((B, H, gs), name, frac)
        assert max(len(set(r.tolist())) for r in sc) >= 3 and max(len(set(col.tolist())) for col in sc.t()) >= 2


def test_attention_scales_and_production_margin():
    """The dense scale times the kernel's fp32 log2(e) is exactly 2^-3; at the production scale 80^-0.5 the dominant-key output
    still rounds to v in both 16-bit types (ED.att_production_margin emulates the two roundings)."""
    import numpy as np
    assert np.float32(ED.ATT_SCALE_DENSE) * ED.ATT_LOG2E == np.float32(2.0 ** -3)
    B, H, gs = ED.ATT_PRODUCTION
    case = ED.attention_case(B, H, ED.ATT_T, gs)
    for dt in (torch.bfloat16, torch.float16):
        c, res, delta = ED.att_production_margin(case, ED.ATT_HD ** -0.5, dt)
        assert abs(res) <= 2.0 ** -14 and delta < 3e-5


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


# ------------------------------------------------------------------------------------------------ LayerNorm
VALUE_FAULT, SCALE_FAULT = 0.40, 0.20        # row dependence of the LayerNorm data is one sign: about 0.5 is the ceiling


def _ln_nwaves(M, cus=ED.LN_HOST_CUS):
    """Row stride of the production row kernel: the waves of its grid (rows per wave ceil(M / (16 CUs)), four waves a workgroup)."""
    rpw = -(-M // (16 * cus))
    return -(-(-(-M // rpw)) // 4) * 4


def pieces_0_1_swapped(D):                     # two 256-column pieces change places
    c = _ar(D)
    return torch.where(c < 256, c + 256, torch.where(c < 512, c - 256, c)) if D >= 512 else c


def pair_swap_lost(D):
    """The 16-byte store without the exchange inside lane pairs: columns 4l+4..4l+7 of piece j (the odd lane's) change places
    with columns 4l..4l+3 of piece j+1 (the even lane's), l even, for every pair of whole pieces j, j+1 (j even)."""
    c = _ar(D)
    piece, lane, e = c // 256, (c % 256) // 4, c % 4
    paired = (piece // 2 * 2 + 1) * 256 + 255 < D
    up = paired & (piece % 2 == 0) & (lane % 2 == 1)          # (j, odd lane) takes (j+1, lane - 1)
    down = paired & (piece % 2 == 1) & (lane % 2 == 0)        # (j+1, even lane) takes (j, lane + 1)
    return torch.where(up, (piece + 1) * 256 + (lane - 1) * 4 + e, torch.where(down, (piece - 1) * 256 + (lane + 1) * 4 + e, c))


# (name, where it acts: "x" = the rows / columns the kernel loads, "y" = where it stores; axis; map taking (size, M))
LN_FAULTS = [
    ("row r takes row r - 1", "y", 0, lambda n, M: rotated(-1)(n)),
    ("row r takes row r - nwaves", "y", 0, lambda n, M: rotated(-_ln_nwaves(M))(n)),
    ("loaded columns shifted by 4", "x", 1, lambda n, M: rotated(4)(n)),
    ("stored columns shifted by 4", "y", 1, lambda n, M: rotated(4)(n)),
    ("loaded 256-column pieces 0 and 1 exchanged", "x", 1, lambda n, M: pieces_0_1_swapped(n)),
    ("stored 256-column pieces 0 and 1 exchanged", "y", 1, lambda n, M: pieces_0_1_swapped(n)),
    ("lane-pair swap of the 16-byte store lost", "y", 1, lambda n, M: pair_swap_lost(n)),
]


def _ln_value_catalogue(M, D):
    x, gamma, beta, y = ED.ln_case(M, D)
    seen, low = set(), []
    for name, op, axis, fn in LN_FAULTS:
        m = fn((M, D)[axis], M)
        if _is_identity(m):
            continue
        if op == "y":
            bad = y.index_select(axis, m)
        elif M * D <= 1 << 20:
            bad = ED.ln_reference(x.index_select(axis, m), gamma, beta, ED.LN_EPS)
        else:                                   # a permutation of a row's columns keeps mean and variance: the closed form holds
            bad = (x.index_select(axis, m) - x.mean(1, keepdim=True)).double() * gamma.double() + beta.double()
        moved = (m != _ar(m.numel())).nonzero()[:, 0]         # the fraction is taken over the rows / columns the fault moves
        frac = float((bad != y).index_select(axis, moved).float().mean())
        seen.add(name)
        if not frac >= VALUE_FAULT:
            low.append((name, round(frac, 4)))
    return seen, low


def test_ln_data_sees_every_fault():
    """Every row, column, piece and lane-pair fault changes at least 40 % of the LayerNorm outputs it moves at every (M, D) the
    exact GPU test runs (the builder itself asserts balance, mean, rstd = 1 and the 16-bit exactness of y at each of them)."""
    met, bad = set(), []
    for (M, D) in ED.ln_shapes():
        seen, low = _ln_value_catalogue(M, D)
        met |= seen
        if low:
            bad.append(((M, D), low))
    assert not bad, bad
    assert met == {f[0] for f in LN_FAULTS}


def test_ln_data_properties():
    """Rows balanced; rstd exactly 1 and y the closed form under the fp32 emulation; y exact in bf16 and fp16; a constant row
    gives beta bit for bit; F.layer_norm is NOT the reference (it is not bit-exact on this data at every D)."""
    for (M, D) in [(5, 4), (5, 96), (197, 256), (197, 1280), (7, 2048)]:
        x, gamma, beta, y = ED.ln_case(M, D)
        pair = x[:, :D // 2] + x[:, D // 2:]                       # column c and column c + D / 2 are m_r +- 0.5
        assert torch.equal(pair, pair[:, :1].expand_as(pair)) and torch.equal(pair[:, :1] / 2, x.mean(1, keepdim=True))
        assert torch.equal((x - pair[:, :1] / 2).abs(), torch.full((M, D), 0.5))
        emu, mean, rstd = ED.ln_emulate(x, gamma, beta, ED.LN_EPS)
        assert torch.equal(rstd, torch.ones(M, 1)) and torch.equal(emu.double(), y)
        assert torch.equal(y.float().bfloat16().double(), y) and torch.equal(y.float().half().double(), y)
        n = y * 16                                                 # an odd integer of at most 5 bits times 2^(k + 3), k = -3..3
        assert torch.equal(n, n.round()) and float(y.abs().max()) <= 15.5 * 8 and float(y.abs().min()) >= 0.5 / 8
        xc = x.clone()
        xc[M // 2] = 3.0
        assert torch.equal(ED.ln_emulate(xc, gamma, beta, ED.LN_EPS)[0][M // 2], beta)
        assert torch.equal(ED.ln_reference(xc, gamma, beta, ED.LN_EPS)[M // 2], beta.double())
    # the data is a pure function of the shape, and differs between shapes
    assert torch.equal(ED.ln_case(5, 96)[0], ED.ln_case(5, 96)[0]) and not torch.equal(ED.ln_case(5, 96)[0][:3], ED.ln_case(3, 96)[0])


def test_ln_accum_data_sees_every_fault():
    """A slab dropped or added twice and the bias dropped change at least 40 % of the accumulated x and of its LayerNorm, at
    every (M, D, S) of the exact hm_layernorm_accum test; the operands are multiples of 0.5 whose sum is the ln_case row."""
    for D in ED.LN_ACCUM_D:
        for M in ED.LN_ACCUM_M:
            for S in ED.LN_ACCUM_S:
                for bias in (True, False):
                    x0, parts, b, x, gamma, beta, y = ED.ln_accum_case(M, D, S, bias)
                    assert parts.shape == (S, M, D) and (b is None) == (not bias)
                    for t in (x0, parts) + ((b,) if bias else ()):
                        assert torch.equal(t * 2, (t * 2).round())
                    bsum = b if bias else torch.zeros(D)
                    assert torch.equal(x0 + (bsum + parts.sum(0)), x)              # in fp32, in the kernel's grouping
                    faults = [("first slab dropped", x - parts[0]), ("last slab dropped", x - parts[S - 1]),
                              ("first slab added twice", x + parts[0]), ("last slab added twice", x + parts[S - 1])]
                    if bias:
                        faults.append(("bias dropped", x - b))
                    for name, xf in faults:
                        fx = float((xf != x).float().mean())
                        fy = float((ED.ln_reference(xf, gamma, beta, ED.LN_EPS) != y).float().mean())
                        assert fx >= VALUE_FAULT and fy >= VALUE_FAULT, ((M, D, S, bias), name, fx, fy)


def test_ln_mx8_scales_see_every_fault():
    """The E8M0 bytes of the quantised closed form depend on the block AND on the row: written [M][D/32], or taken from the
    neighbouring block or row, at least 20 % of them change; with more than one block and more than two rows they take two
    values along the rows of some block and min(3, blocks) values along the blocks of some row."""
    from oracle import fp8_ref as Q
    met, lo, hi = set(), 255, 0
    for D in ED.LN_MX8_D:
        for M in ED.LN_MX8_M:
            y = ED.ln_case(M, D)[3].float()
            q, sc = Q.mx8_quantize(y)
            nblk = D // 32
            assert sc.shape == (nblk, M)
            lo, hi = min(lo, int(sc.min())), max(hi, int(sc.max()))
            assert torch.equal(Q.mx8_quantize(y)[0], q)
            faults = [("scales written [M][D/32]", sc.t().contiguous().view(nblk, M), nblk > 1 and M > 1),
                      ("scale of the neighbouring block", sc.roll(1, 0), nblk > 1),
                      ("scale of the neighbouring row", sc.roll(1, 1), M > 1)]
            for name, bad, applies in faults:
                if not applies:
                    continue
                met.add(name)
                frac = float((bad != sc).float().mean())
                assert frac >= SCALE_FAULT, ((M, D), name, frac)
            if nblk > 1 and M > 2:
                assert max(len(set(r.tolist())) for r in sc) >= 2, (M, D)
                assert max(len(set(c.tolist())) for c in sc.t()) >= min(3, nblk), (M, D)
            if M >= 197:
                assert all(len(set(r.tolist())) >= 2 for r in sc), (M, D)
    assert len(met) == 3 and 116 <= lo and hi <= 126 and hi - lo >= 8, (lo, hi)


def _ln_one_pass(x, gamma, beta, eps):
    D = x.shape[1]
    mean = x.sum(1, keepdim=True) / D
    return (x - mean) / torch.sqrt((x * x).sum(1, keepdim=True) / D - mean * mean + eps) * gamma + beta


def _ln_two_pass(x, gamma, beta, eps, rstd):
    D = x.shape[1]
    d = x - x.sum(1, keepdim=True) / D
    return d * rstd((d * d).sum(1, keepdim=True) / D, eps) * gamma + beta


def _hostile(D, eps):
    x, gamma, beta, kind = ED.ln_hostile_rows(D, eps)
    return x, gamma, beta, kind, ED.ln_reference(x, gamma, beta, eps)


def _row_err(got, ref):
    return torch.nan_to_num((got.double() - ref).abs().amax(1, keepdim=True), nan=float("inf"))


def test_ln_error_multiples_are_the_measured_ones():
    """ED.LN_MULTIPLES states, per kind of row, the largest error of the fp32 two-pass emulation against fp64 in units of
    ED.ln_error_unit.  Measured here over D in {96, 320, 1280, 2048} and eps in {1e-6, 1e-5}: uniform 1.52, mean 1000 0.95,
    mean -3000 0.80, variance = eps 1.69, variance = 1e-3 eps 2.28, one outlier of 1e4 1.86, all-zero row 0 (error 0).  The table
    holds them rounded up; it may neither be exceeded nor be twice what is measured."""
    worst = torch.zeros(len(ED.LN_HOSTILE_KINDS), dtype=torch.float64)
    for D in ED.LN_HOSTILE_D:
        for eps in ED.LN_HOSTILE_EPS:
            x, gamma, beta, kind, ref = _hostile(D, eps)
            assert float(x.abs().max()) <= 1e4
            err = _row_err(ED.ln_emulate(x, gamma, beta, eps)[0], ref)
            unit = ED.ln_error_unit(x, gamma, eps)
            zero = kind == ED.LN_HOSTILE_KINDS.index("zero")
            assert float(err[zero].max()) == 0.0 and float(unit[zero].max()) == 0.0
            assert (err <= ED.ln_error_bound(x, gamma, eps, kind, margin=1.0)).all(), (D, eps)
            ratio = torch.where(zero[:, None], torch.zeros_like(err), err / unit.clamp_min(1e-300))
            worst = torch.maximum(worst, torch.stack([ratio[kind == i].max() for i in range(len(worst))]))
    for i, k in enumerate(ED.LN_HOSTILE_KINDS):
        assert float(worst[i]) <= ED.LN_MULTIPLES[k] <= 2 * float(worst[i]), (k, float(worst[i]))
    assert ED.LN_KERNEL_MARGIN == 4.0


def test_ln_error_bound_separates_wrong_formulas():
    """The bound the GPU accuracy test gives the kernels (4 x the measured multiples) against three wrong LayerNorms, on the
    CPU in fp32: a one-pass E[x^2] - mean^2 variance misses it by >= 100 x on the worst row of each large-mean kind, and an
    eps added outside the square root, or left out, by >= 100 x on EVERY row whose variance is eps or 1e-3 eps."""
    kinds = ED.LN_HOSTILE_KINDS
    for D in ED.LN_HOSTILE_D:
        for eps in ED.LN_HOSTILE_EPS:
            x, gamma, beta, kind, ref = _hostile(D, eps)
            bound = ED.ln_error_bound(x, gamma, eps, kind)
            over = _row_err(_ln_one_pass(x, gamma, beta, eps), ref) / bound
            for k in ("mean_1000", "mean_-3000"):
                assert float(over[kind == kinds.index(k)].max()) >= 100, (D, eps, k)
            outside = _ln_two_pass(x, gamma, beta, eps, lambda var, e: 1.0 / (torch.sqrt(var) + e))
            dropped = _ln_two_pass(x, gamma, beta, eps, lambda var, e: 1.0 / torch.sqrt(var))
            for got in (outside, dropped):
                over = _row_err(got, ref) / bound
                for k in ("var_eps", "var_1e-3_eps"):
                    assert float(over[kind == kinds.index(k)].min()) >= 100, (D, eps, k)
            right = _ln_two_pass(x, gamma, beta, eps, lambda var, e: 1.0 / torch.sqrt(var + e))
            assert (_row_err(right, ref) <= bound / ED.LN_KERNEL_MARGIN).all()


def test_ln_builders_refuse_data_that_is_not_exact(monkeypatch):
    monkeypatch.setattr(ED, "LN_EPS", 0.5)                       # rstd = 1 / sqrt(0.75): the closed form no longer holds
    with pytest.raises(AssertionError):
        ED.ln_case(5, 96)
    monkeypatch.setattr(ED, "LN_EPS", 0.75)
    monkeypatch.setattr(ED, "LN_PEAK_GAMMA", 4097)               # y needs more bits than bf16 has
    with pytest.raises(AssertionError):
        ED.ln_case(5, 96)


# ------------------------------------------------------------------------------------------------ SAR hand-mesh head
def k32_tiles_rotated(K):                      # the K loop of csrc/sar.hip and csrc/sar_f32.hip is 32 wide
    k = _ar(K)
    return ((k // 32 + 1) % (K // 32)) * 32 + k % 32 if K >= 64 else k


def k32_tail_is_first(K):                      # the last 32 k read from the first 32's slot
    k = _ar(K)
    return torch.where(k >= K - 32, k % 32, k)


def k_halves_of_8_swapped(K):                  # k rows q and q + 4 of a group of 8: the two transposed reads of the [K][N] operand
    return _ar(K) ^ 4


def _xor_inside(bits):
    def fn(n):
        m = _ar(n) ^ bits
        return torch.where(m < n, m, _ar(n))
    return fn


# "W" is the NT operand [N][K]; for L . X it is the transpose of the row-major [K][N] operand: its rows are that operand's columns
SAR_GEMM_FAULTS = [f for f in GEMM_FAULTS if f[1] != "resid"] + [
    ("W: 32-wide K-tiles rotated by one", "w", 1, k32_tiles_rotated),
    ("X: 32-wide K-tiles rotated by one", "x", 1, k32_tiles_rotated),
    ("W: last 32 k replaced by the first 32", "w", 1, k32_tail_is_first),
    ("X: last 32 k replaced by the first 32", "x", 1, k32_tail_is_first),
    ("W: k rows q and q + 4 swapped inside groups of 8", "w", 1, k_halves_of_8_swapped),
    ("W rows (columns of [K][N]) reversed inside groups of 4", "w", 0, _xor_inside(3)),
    ("W rows (columns of [K][N]): the 4-wide blocks of a group of 16 reversed", "w", 0, _xor_inside(12)),
    ("W rows (columns of [K][N]) rotated by 64", "w", 0, rotated(64)),
]


def _sar_gemm_catalogue(x, w, bias, finish, faults=None):
    """The catalogue on finish(x w^T + bias), on the module's 256 x 256 spread of outputs: (faults met, faults below the bar)."""
    faults = SAR_GEMM_FAULTS if faults is None else faults
    ops = {"x": x, "w": w, "bias": bias}
    rows, cols = _spread(x.shape[0]), _spread(w.shape[0])
    sizes = {("x", 0): x.shape[0], ("x", 1): x.shape[1], ("w", 0): w.shape[0], ("w", 1): w.shape[1], ("bias", 0): w.shape[0]}
    _, seen, low = _run_catalogue(faults, ops, lambda maps: finish(_gemm_sub(ops, rows, cols, maps)), sizes)
    return seen, low


def _f16_leaky(v):
    return ED.sar_leaky(v).half()


def test_sar_fc_data_sees_every_fault():
    """Every fault changes more than half of the fp16 LeakyReLU outputs (the coarsest of the four outputs) at every fc shape where
    it is not the identity; at (1, 1, 32) the single output must change."""
    met = set()
    for (M, N, K) in ED.SAR_FC:
        x, w, b, ref = ED.sar_fc_case(M, N, K)
        assert torch.equal(ref["f16_leaky"], _f16_leaky(x @ w.t() + b))
        seen, low = _sar_gemm_catalogue(x, w, b, _f16_leaky)
        assert not low, ((M, N, K), low)
        met |= seen
    assert met == {f[0] for f in SAR_GEMM_FAULTS}, {f[0] for f in SAR_GEMM_FAULTS} - met


def test_sar_mix_data_sees_every_fault():
    """L . X as x = the Laplacian (778, ldl) with its zero columns and w = the [K][N] operand transposed, its k rows 778 .. ldl - 1
    being row 777 again, as the f16 kernel's clamp reads them (they meet the zero columns: the product is the same).  The K faults
    act on all ldl k.  A fault of the [K][N] operand that moves none of its first 778 k rows is no fault, by the contract that
    what lies past them never contributes (the last 32 k at ldl = 832), and is passed over there."""
    met = set()
    for ldl in ED.SAR_MIX_LDL:
        for N in ED.SAR_MIX_N + ED.SAR_MIX_N_F32_ONLY:
            lap, x, y = ED.sar_mix_case(N, ldl)
            assert not lap[:, ED.SAR_NV:].any() and lap.shape == (ED.SAR_NV, ldl)
            wt = x[_ar(ldl).clamp(max=ED.SAR_NV - 1)].t().contiguous()
            assert torch.equal(lap @ wt.t(), y)
            faults = [f for f in SAR_GEMM_FAULTS if not (f[1:3] == ("w", 1) and torch.equal(f[3](ldl)[:ED.SAR_NV], _ar(ED.SAR_NV)))]
            assert len(SAR_GEMM_FAULTS) - len(faults) == (1 if ldl == 832 else 0)
            seen, low = _sar_gemm_catalogue(lap, wt, None, lambda v: v, faults)
            assert not low, ((N, ldl), low)
            met |= seen
    assert met == {f[0] for f in SAR_GEMM_FAULTS if f[1] != "bias"}, {f[0] for f in SAR_GEMM_FAULTS if f[1] != "bias"} - met


def _saigb_graph_variant(v, bias, tmpl, B, fault):
    """The fp16 graph (778, B, 544) with one mistake of the epilogue's scatter."""
    NV = ED.SAR_NV
    if fault == "bias indexed by n instead of m":
        v = v - bias[None, :] + bias[:v.shape[0], None]
    h = _f16_leaky(v)
    if fault == "channels read as [8][778]":
        g = ED.sar_graph(h, tmpl, B)
        g[:, :, :512] = h.reshape(B, 64, 8, NV).permute(3, 0, 2, 1).reshape(NV, B, 512)
        return g
    if fault == "positions and hands transposed ([64][B])":
        g = ED.sar_graph(h, tmpl, B)
        g[:, :, :512] = h.reshape(64, B, NV, 8).permute(2, 1, 3, 0).reshape(NV, B, 512)
        return g
    if fault == "template rotated by one node":
        return ED.sar_graph(h, tmpl.roll(1, 0), B)
    g = ED.sar_graph(h, tmpl, B)
    if fault == "hand-major rows":
        return g.permute(1, 0, 2).contiguous().reshape(NV, B, ED.SAR_KG)
    return g


SAIGB_SCATTER_FAULTS = ["channels read as [8][778]", "positions and hands transposed ([64][B])", "hand-major rows",
                        "template rotated by one node", "bias indexed by n instead of m"]


def test_sar_saigb_data_sees_every_fault():
    """The GEMM catalogue on feat w^T + bias at every (B, K), and the scatter's own faults on the whole graph: each changes more
    than half of the live columns (of the template columns for the template fault).  The two hand faults are the identity at
    B = 1 and are met at B = 3."""
    met, met_scatter = set(), {}
    for (B, K) in ED.SAR_SAIGB:
        feat, w, b, tmpl, v, graphs = ED.sar_saigb_case(B, K)
        ref = _saigb_graph_variant(v, b, tmpl, B, None)
        assert torch.equal(ref, graphs["f16"]) and torch.equal(ED.sar_graph(ED.sar_leaky(v), tmpl, B), graphs["f32"])
        assert not ref[:, :, 515:].any() and torch.equal(ref[:, 0, 512:515].float(), tmpl) and float(tmpl.abs().max()) == 4
        seen, low = _sar_gemm_catalogue(feat, w, b, _f16_leaky)
        assert not low, ((B, K), low)
        met |= seen
        for fault in SAIGB_SCATTER_FAULTS:
            got = _saigb_graph_variant(v, b, tmpl, B, fault)
            live = slice(512, 515) if fault.startswith("template") else slice(0, 515)
            if torch.equal(got, ref):
                assert B == 1 and fault in SAIGB_SCATTER_FAULTS[1:3], (B, K, fault)
                continue
            frac = float((got[:, :, live] != ref[:, :, live]).float().mean())
            assert frac > HALF, (B, K, fault, frac)
            met_scatter.setdefault(fault, set()).add(B)
    assert met == {f[0] for f in SAR_GEMM_FAULTS}
    assert met_scatter == {f: ({3} if f in SAIGB_SCATTER_FAULTS[1:3] else {1, 3}) for f in SAIGB_SCATTER_FAULTS}


# ---- soft-argmax
def _softargmax_model(c, fault=None):
    """mesh2pose + SoftHeatmap + coordinate sums in float64 on the case's operands, with one mistake: (B, 799, 3)."""
    lxy, lz = c["lxy"].double(), c["lz"].double()
    B = lxy.shape[0]
    w_xy, w_z, beta, wx, wy = c["w_xy"].double(), c["w_z"].double(), c["beta"], c["wx"], c["wy"]
    if fault == "mesh2pose W transposed":
        w_xy, w_z = (w.t().contiguous().reshape(w.shape) for w in (w_xy, w_z))
    if fault == "mesh2pose W rotated by one vertex":
        w_xy, w_z = w_xy.roll(1, 1), w_z.roll(1, 1)
    full = [torch.cat([t, torch.einsum("jv,bvc->bjc", w, t) + b.double()[None, :, None]], 1)
            for t, w, b in ((lxy, w_xy, c["b_xy"]), (lz, w_z, c["b_z"]))]
    if fault == "hand and node transposed in the row address":              # the buffers are [799][B][1024]; row b * 799 + n is read
        full = [t.permute(1, 0, 2).contiguous().reshape(B, ED.SAR_NT, ED.SAR_CELLS) for t in full]
    if fault == "beta rotated by one node":
        beta = beta.roll(1)
    if fault is not None and fault.startswith("cells rotated by "):
        by = int(fault.rsplit(" ", 1)[1])
        wx, wy = wx.roll(-by), wy.roll(-by)
    if fault == "the four cells of a lane reversed":
        wx, wy = wx[_ar(ED.SAR_CELLS) ^ 3], wy[_ar(ED.SAR_CELLS) ^ 3]
    out = ED.sar_softmax_reference(full[0], full[1], beta.expand(B, ED.SAR_NT), wx, wy)
    if fault == "output triples node-major":                                # written at (n * B + b) * 3, read as [B][799][3]
        out = out.permute(1, 0, 2).contiguous().reshape(B, ED.SAR_NT, 3)
    return out


# (fault, rows it can reach, bar on the fraction of (hand, node) triples it changes)
SOFTARGMAX_FAULTS = [("cells rotated by 4", "all", HALF), ("cells rotated by 256", "all", HALF), ("cells rotated by 32", "all", HALF),
                     ("the four cells of a lane reversed", "all", HALF), ("hand and node transposed in the row address", "all", HALF),
                     ("output triples node-major", "all", HALF), ("mesh2pose W transposed", "joints", HALF),
                     ("mesh2pose W rotated by one vertex", "joints", HALF), ("beta rotated by one node", "all", 0.25)]


@pytest.mark.parametrize("m2p", ["dense", "onehot"])
def test_sar_softargmax_data_sees_every_fault(m2p):
    """Each fault changes more than half of the (hand, node) triples it can reach (the mesh2pose faults reach the 21 joint rows;
    beta rotated by one node changes only rows whose beta moves to or from 0, 3/8 of them in expectation: the bar is a quarter);
    cells rotated by 32 changes more than half of the y values.  The two hand / node faults are the identity at B = 1."""
    met = {}
    for B in ED.SAR_SOFTARGMAX_B:
        c = ED.sar_softargmax_case(B, m2p)
        ref = _softargmax_model(c)
        assert float((ref - c["coords"]).abs().max()) < 1e-12                 # exp(-256) is not 0 in float64: 1e-111
        for fault, reach, bar in SOFTARGMAX_FAULTS:
            got = _softargmax_model(c, fault)
            rows = slice(ED.SAR_NV, ED.SAR_NT) if reach == "joints" else slice(0, ED.SAR_NT)
            if torch.equal(got, ref):
                assert B == 1 and fault in ("hand and node transposed in the row address", "output triples node-major"), (B, fault)
                continue
            frac = float((got[:, rows] != ref[:, rows]).any(-1).float().mean())
            assert frac > bar, (B, m2p, fault, frac)
            if fault == "cells rotated by 32":
                assert float((got[:, :, 1] != ref[:, :, 1]).float().mean()) > HALF
            met.setdefault(fault, set()).add(B)
    assert set(met) == {f[0] for f in SOFTARGMAX_FAULTS} and all(3 in v for v in met.values())


def test_sar_softargmax_data_is_exact():
    """The fp32 rule (tests/sar_rule.py: tail) reproduces the closed form bit for bit: every row of the one-hot case, the
    vertex rows of the dense one (its joint rows within 1e-6); the supports are spread: most rows have their own (x, y)."""
    import sar_rule as R
    for m2p, B in (("dense", 1), ("dense", 3), ("onehot", 3)):
        c = ED.sar_softargmax_case(B, m2p)
        sd = {"head.gbbmr.mesh2pose_hm.weight": c["w_xy"], "head.gbbmr.mesh2pose_hm.bias": c["b_xy"],
              "head.gbbmr.mesh2pose_dm.weight": c["w_z"], "head.gbbmr.mesh2pose_dm.bias": c["b_z"],
              "head.gbbmr.soft_heatmap.beta.weight": c["beta"], "head.gbbmr.soft_heatmap.wx": c["wx"].view(32, 32),
              "head.gbbmr.soft_heatmap.wy": c["wy"].view(32, 32)}
        got = R.tail(sd, c["lxy"], c["lz"]).double()
        exact = slice(0, ED.SAR_NT if m2p == "onehot" else ED.SAR_NV)
        assert torch.equal(got[:, exact], c["coords"][:, exact]), m2p
        assert float((got - c["coords"]).abs().max()) < 1e-6
        xy = c["coords"][:, :ED.SAR_NV, :2].reshape(-1, 2)
        assert len({tuple(r) for r in xy.tolist()}) > HALF * xy.shape[0]         # (the quarter of the rows with beta = 0 share one answer)
        assert set(c["beta"].tolist()) == set(ED.SAR_BETAS) and set(c["beta"][ED.SAR_NV:].tolist()) == set(ED.SAR_BETAS)


# ---- post-processing
def _post_hands(**change):
    """SAR_POST_HANDS with each field named in `change` taken from the next hand: hand b gets that of hand b + 1."""
    hands = [dict(h) for h in ED.SAR_POST_HANDS]
    n = len(hands)
    for k in change:
        for b in range(n):
            hands[b][k] = ED.SAR_POST_HANDS[(b + 1) % n][k]
    return hands


def _post_neighbour_offsets():
    """Every hand with a map takes the depth offset of the next hand with a map (its own width and height)."""
    hands = [dict(h) for h in ED.SAR_POST_HANDS]
    with_map = [b for b, h in enumerate(hands) if h["map"] is not None]
    for i, b in enumerate(with_map):
        hands[b]["off"] = ED.SAR_POST_MAPS[hands[with_map[(i + 1) % len(with_map)]]["map"]][0]
    return hands


def test_sar_post_data_sees_every_fault():
    """Each fault changes more than half of the values it can reach: (hands, columns of [u, v, d, x, y, z]).  A root reaches d and
    all of xyz; the flip reaches u and x; the sampling faults reach the hands whose row 778 lands inside or across a border of
    its map (outside, every variant samples 0)."""
    coords, depth, hands, uvd, xyz = ED.sar_post_case()
    ref = torch.cat([uvd, xyz], 2).double()
    B = ED.SAR_POST_B
    flipped = [b for b, h in enumerate(hands) if h["flip"]]
    rooted = [b for b, h in enumerate(hands) if h["map"] is None]
    sampled = [b for b, h in enumerate(hands) if h["lands"] in ("inside", "border")]
    assert len(flipped) == 2 and len(rooted) == 2 and len(sampled) == 2 and set(flipped) & set(sampled) and set(flipped) & set(rooted)
    Z = [2, 3, 4, 5]
    every = {k: True for k in ("t", "box", "flip", "map")}      # the fields of hm_sar_hand; root[b] and the coordinates stay
    table = [
        ("hand structs rotated by one", dict(hands=_post_hands(**every)), range(B), range(6)),
        ("root rotated", dict(hands=_post_hands(root=True)), rooted, Z),
        ("flip ignored", dict(fault="flip ignored"), flipped, [0, 3]),
        ("row 778 un-flipped before sampling", dict(fault="row 778 un-flipped before sampling"), sorted(set(flipped) & set(sampled)), Z),
        ("depth offset of the neighbouring hand", dict(hands=_post_neighbour_offsets()), sampled, Z),
        ("x and y of the sample swapped", dict(fault="x and y of the sample swapped"), sampled, Z),
        ("depth_w and depth_h swapped", dict(fault="depth_w and depth_h swapped"), sampled, Z),
    ]
    for name, kw, hs, cols in table:
        u2, x2, _ = ED.sar_post_expect(coords, depth, **kw)
        got = torch.cat([u2, x2], 2)
        frac = float((got[list(hs)][:, :, list(cols)] != ref[list(hs)][:, :, list(cols)]).float().mean())
        assert frac > HALF, (name, frac)
    # with neither, or with one source taken away, the roots are the ones the GPU test expects
    assert ED.sar_post_expect(coords, depth, with_depth=False)[2] == [h["root"] for h in hands]
    r = ED.sar_post_expect(coords, depth, with_root=False)[2]
    assert [r[b] for b in rooted] == [0.0, 0.0] and r[[b for b, h in enumerate(hands) if h["lands"] == "outside"][0]] == 0.0
    assert all(r[b] > 0 for b in sampled) and len({h["root"] for h in hands}) == B


def test_sar_post_data_is_exact():
    """The float64 formulas of ED.sar_post_expect are fp32 values (asserted by the builder) and are reproduced by the fp32 rule
    (tests/sar_rule.py: post_process) bit for bit, the sampled roots by F.grid_sample in float64 on the un-flipped row 778."""
    import numpy as np
    import sar_rule as R
    Wi, Hi = ED.SAR_POST_IMG
    fx, fy, cu, cv = ED.SAR_POST_K
    K = np.array([[fx, 0, cu], [0, fy, cv], [0, 0, 1]])
    for with_root, with_depth in ((True, True), (True, False), (False, True)):
        coords, depth, hands, uvd, xyz = ED.sar_post_case(with_root, with_depth)
        _, _, roots = ED.sar_post_expect(coords, depth, with_root=with_root, with_depth=with_depth)
        for b, h in enumerate(hands):
            t = np.array(h["t"], np.float32)
            if h["map"] is not None and with_depth:
                off, W, H = ED.SAR_POST_MAPS[h["map"]]
                fu, fv = (torch.tensor(h["t"], dtype=torch.float64) @ torch.tensor([h["uv"][0], h["uv"][1], 1.0], dtype=torch.float64)).tolist()
                grid = torch.tensor([[[[fu / (Wi // 2) - 1, fv / (Hi // 2) - 1]]]], dtype=torch.float64)
                d = depth[off:off + W * H].double().reshape(1, 1, H, W)
                assert float(F.grid_sample(d, grid, mode="bilinear", padding_mode="zeros", align_corners=False)) == roots[b], b
            assert np.float32(roots[b]) == roots[b]
            out = R.post_process(coords[b].numpy(), np.float32(roots[b]), t, K, Wi, bool(h["flip"]), depth_box=h["box"], P=ED.SAR_POST_P)
            assert out["mesh_uvd"].dtype == np.float32 and out["mesh_xyz"].dtype == np.float32
            assert np.array_equal(np.concatenate([out["mesh_uvd"], out["pose_uvd"]]), uvd[b].numpy()), b
            assert np.array_equal(np.concatenate([out["mesh_xyz"], out["pose_xyz"]]), xyz[b].numpy()), b


def test_sar_builders_refuse_data_that_is_not_exact(monkeypatch):
    monkeypatch.setattr(ED, "F16_EXACT_INT", 256.0)              # the production fc sums pass 256
    with pytest.raises(AssertionError):
        ED.sar_fc_case(778, 1024, 1024)
    with pytest.raises(AssertionError):
        ED.sar_mix_case(544, 800)
    monkeypatch.undo()
    monkeypatch.setattr(ED, "SAR_BETAS", [0.0, 0.25, 0.5, 1.0])  # beta (l - 256 - l) = -64: exp is no longer 0
    with pytest.raises(AssertionError):
        ED.sar_softargmax_case(1, "onehot")
    monkeypatch.undo()
    monkeypatch.setattr(ED, "SAR_M2P_SALT", 0)                   # a dense joint row with three tied maxima
    with pytest.raises(AssertionError):
        ED.sar_softargmax_case(1, "dense")
    monkeypatch.undo()
    monkeypatch.setattr(ED, "SAR_POST_K", (1000.0, 512.0, 512.0, 256.0))      # a focal length that is no power of two
    with pytest.raises(AssertionError):
        ED.sar_post_case()


# ------------------------------------------------------------------------------------------------ MANO tail
def _rows_changed(got, ref, width):
    return (got.reshape(-1, width) != ref.reshape(-1, width)).any(1)


MANO_CASES = [(B, V, False) for B in ED.MANO_B for V in ED.MANO_V] + [ED.MANO_DEGENERATE + (True,)]
# fault -> the output it concerns and the width of one of its rows
MANO_CONCERNS = {"wrong parent table": ("joints", 3), "joint map rotated": ("joints", 3), "tips off by one": ("joints", 3),
                 "posedirs as [3V][135]": ("verts", 3), "shapedirs as [10][3V]": ("verts", 3), "rotation transposed": ("rotmats", 9),
                 "pose feature from joint 0": ("verts", 3), "lbs_weights as [16][V]": ("verts", 3), "joints from v_posed": ("joints", 3),
                 "A without G J": ("verts", 3), "one range unposed": ("verts", 3), "child before parent": ("joints", 3),
                 "cam columns rotated": ("kp2d", 2)}


@pytest.mark.parametrize("B,V,degenerate", MANO_CASES)
def test_mano_data_is_exact_and_sees_every_fault(B, V, degenerate):
    """mano_rule's stage assertions hold on the case (they run inside the call), and each fault of MANO_FAULTS changes more
    than half of the rows of the output it concerns: all five tip joints of every hand for the tip fault, more than half of
    the unposed range for the one-range fault, every cam_t row as well for the camera fault."""
    from hamer_yolo_amd import synth
    mp, pose, betas, cam, _ = ED.mano_exact_case(B, V, degenerate=degenerate)
    ref = ED.mano_rule(mp, pose, betas, cam)
    assert set(MANO_CONCERNS) == set(ED.MANO_FAULTS)
    tip_rows = torch.tensor([i for i, s in enumerate(synth.MANO_JOINT_MAP) if s >= 16])
    for fault in ED.MANO_FAULTS:
        got = ED.mano_rule(mp, pose, betas, cam, fault=fault, exact=False)
        key, width = MANO_CONCERNS[fault]
        changed = _rows_changed(got[key], ref[key], width).reshape(B, -1)
        if fault == "tips off by one":
            assert bool(changed[:, tip_rows].all()) and not bool(_rows_changed(got["verts"], ref["verts"], 3).any()), (fault, B, V)
            continue
        if fault == "one range unposed":
            lo, hi = ED.mano_ranges(V)[ED.MANO_UNPOSED_RANGE]
            assert float(changed[:, lo:hi].float().mean()) > HALF and not bool(changed[:, :lo].any()) and not bool(changed[:, hi:].any())
            continue
        assert float(changed.float().mean()) > HALF, (fault, B, V, float(changed.float().mean()))
        if fault == "cam columns rotated":
            assert bool(_rows_changed(got["cam_t"], ref["cam_t"], 3).all())


def test_mano_case_is_what_the_issue_asks_for():
    """Rotations: all 24 proper signed permutations occur, every joint differs from all its ancestors, hands 0 and 1 differ at
    every joint; the 6-D codes are not normalised and half of them carry a t e_i term; the camera rows give tz = 2^m but for
    the one row with c0 = 0; the tips are owned as MANO_TIP_OWNER says at every V."""
    import numpy as np
    from hamer_yolo_amd import synth
    from hamer_yolo_amd.hamer.utils.geometry import rot6d_to_rotmat
    table, sym = ED.mano_rotation_table()
    assert len(set(table)) == 24 and sum(sym) == 10
    seen = set()
    for B, V, _ in MANO_CASES[:-1]:
        mp, pose, betas, cam, rot = ED.mano_exact_case(B, V)
        seen |= set(rot.reshape(-1).tolist())
        for j in range(1, 16):
            a = synth.MANO_PARENTS[j]
            while a >= 0:
                assert bool((rot[:, j] != rot[:, a]).all())
                a = synth.MANO_PARENTS[a]
        assert B == 1 or bool((rot[0] != rot[1]).all())
        x = pose.reshape(B * 16, 6)
        n1, dot = x[:, :3].norm(dim=1), (x[:, :3] * x[:, 3:]).sum(1)
        assert B == 1 or (float((n1 != 1).float().mean()) > HALF and 0.25 < float((dot != 0).float().mean()) < 0.75)
        R = ED.mano_rot6d_rule(pose).reshape(B, 16, 3, 3)
        assert torch.equal(R.float(), rot6d_to_rotmat(pose).reshape(B, 16, 3, 3))             # the project's CPU reference, bit for bit
        assert torch.equal(R @ R.transpose(-1, -2), torch.eye(3, dtype=torch.float64).expand(B, 16, 3, 3))
        out = ED.mano_rule(mp, pose, betas, cam)
        tz = out["cam_t"][:, 2].double()
        zero = cam[:, 0] == 0
        assert int(zero.sum()) == (1 if B > 1 else 0)
        assert torch.equal(tz[~zero], 2 * ED.MANO_FOCAL / (ED.MANO_IMAGE * cam[~zero, 0].double())) and torch.equal(torch.log2(tz[~zero]), torch.log2(tz[~zero]).round())
        assert not bool(zero.any()) or float(tz[zero]) == float(np.float32(10000.0) / np.float32(1e-9))
        assert bool(out["kp2d"].isfinite().all()) and (B == 1 or float((out["kp2d"] != 0).float().mean()) > 0.9)
        owner = [next(k for k, (lo, hi) in enumerate(ED.mano_ranges(V)) if lo <= t < hi) for t in synth.MANO_TIP_VERTS]
        assert tuple(owner) == ED.MANO_TIP_OWNER
    assert seen == set(range(24))
    assert ED.mano_ranges(745)[3] == (561, 745) and ED.mano_ranges(800)[3] == (600, 800)


def test_mano_degenerate_poses_are_exact():
    """a1 = 0 gives columns (0, a2 / |a2|, 0) and a2 = t a1 gives (a1 / |a1|, 0, 0): the rule, with the kernel's floor of 1e-12f,
    equals the project's rot6d_to_rotmat on the CPU, and the whole forward stays exact (the stage assertions run)."""
    from hamer_yolo_amd.hamer.utils.geometry import rot6d_to_rotmat
    B, V = ED.MANO_DEGENERATE
    mp, pose, betas, cam, _ = ED.mano_exact_case(B, V, degenerate=True)
    out = ED.mano_rule(mp, pose, betas, cam)
    R = out["rotmats"]
    assert torch.equal(R, rot6d_to_rotmat(pose).reshape(B, 16, 3, 3) + 0.0)
    b, j = ED.MANO_DEGENERATE_JOINTS["a1 = 0"]
    assert not bool(pose.reshape(B, 16, 6)[b, j, :3].any())
    assert not bool(R[b, j, :, 0].any()) and not bool(R[b, j, :, 2].any()) and float(R[b, j, :, 1].abs().sum()) == 1
    b, j = ED.MANO_DEGENERATE_JOINTS["a2 = t a1"]
    assert torch.equal(pose.reshape(B, 16, 6)[b, j, 3:], 1.5 * pose.reshape(B, 16, 6)[b, j, :3])
    assert float(R[b, j, :, 0].abs().sum()) == 1 and not bool(R[b, j, :, 1:].any())
    plain = ED.mano_rule(*ED.mano_exact_case(B, V)[:4])
    assert float(_rows_changed(out["verts"][0], plain["verts"][0], 3).float().mean()) > HALF      # the degenerate joints reach the mesh


def test_mano_builders_refuse_data_that_is_not_exact():
    mp, pose, betas, cam, _ = ED.mano_exact_case(5, 778)
    bad = dict(mp, v_template=mp["v_template"] + 1.0 / 3)
    with pytest.raises(AssertionError):
        ED.mano_rule(bad, pose, betas, cam)
    with pytest.raises(AssertionError):
        ED.mano_rule(mp, pose, betas * 2.0 ** 22, cam)                   # multiples of the quantum, but past 2^24 of them
    tilted = pose.clone()
    tilted[0, :3] = 1.0                                            # a1 = (1, 1, 1): its norm is no fp32 value
    with pytest.raises(AssertionError):
        ED.mano_rule(mp, tilted, betas, cam)
    with pytest.raises(AssertionError):
        ED.mano_rule(mp, pose, betas, cam + torch.tensor([1e-3, 0.0, 0.0]))      # image_size * c0 is no longer exact


# ------------------------------------------------------------------------------------------------ Detect decode
def test_decode_sigmoid_has_three_exact_values():
    import numpy as np
    f = np.float32
    with np.errstate(over="ignore"):
        assert np.exp(f(128.0)) == np.inf and np.exp(f(-128.0)) == 0 and np.exp(f(128.0)).dtype == f
        vals = [f(1) / (f(1) + np.exp(-f(r))) for r in (0.0, 128.0, -128.0)]
    assert vals == [0.5, 1.0, 0.0] and all(v.dtype == f for v in vals)
    assert ED.sigmoid_f32(torch.tensor([0.0, 128.0, -128.0])).tolist() == [0.5, 1.0, 0.0]


def _decode_applies(fault, nb, ny, nx, row0):
    if fault in ("x and y grid swapped", "anchor w and h swapped"):
        return (ny, nx) != (1, 1)
    if fault == "rows in (y, x, a) order":
        return ny * nx > 1                                               # the identity map on a single cell
    if fault == "row0 ignored":
        return row0 != 0
    if fault in ("raw image stride zero", "pred image stride zero"):
        return nb > 1
    return True


def test_decode_data_is_exact_and_sees_every_fault():
    """Every case of the exact GPU test: the rule's values are short dyadic fp32 numbers (asserted inside), and every fault that
    applies changes more than half of the rows it concerns -- the rows the right or the wrong decode writes; images 1.. for the
    image-stride faults.  Every grid meets all three anchor levels and every fault applies somewhere."""
    met, levels = set(), {}
    cases = ED.decode_cases()
    assert len(cases) == len(set(cases)) == 96
    for nb, ny, nx, nc, ldraw, row0, rows, level in cases:
        levels.setdefault((ny, nx), set()).add(level)
        raw = ED.decode_exact_case(nb, ny, nx, nc, ldraw, row0, rows)
        assert bool(raw[:, :, 3 * (5 + nc):].isnan().all()) and set(raw[:, :, :3 * (5 + nc)].reshape(-1).tolist()) <= {0.0, 128.0, -128.0}
        s = ED.sigmoid_f32(raw)
        ref = ED.decode_rule(s, ny, nx, nc, row0, rows, level)
        n = 3 * ny * nx
        assert bool((ref[:, :row0] == ED.DECODE_SENTINEL).all()) and bool((ref[:, row0 + n:] == ED.DECODE_SENTINEL).all())
        assert not bool((ref[:, row0:row0 + n] == ED.DECODE_SENTINEL).any()) and rows > row0 + n
        for fault in ED.DECODE_FAULTS:
            if not _decode_applies(fault, nb, ny, nx, row0):
                continue
            got = ED.decode_rule(s, ny, nx, nc, row0, rows, level, fault=fault, exact=False)
            first = 1 if "image stride" in fault else 0
            touched = ((ref != ED.DECODE_SENTINEL) | (got != ED.DECODE_SENTINEL)).any(2)[first:]
            changed = (ref != got).any(2)[first:]
            frac = float(changed[touched].float().mean())
            assert frac > HALF, (fault, nb, ny, nx, nc, ldraw, row0, level, frac)
            met.add(fault)
    assert met == set(ED.DECODE_FAULTS) and all(v == {0, 1, 2} for v in levels.values())


def test_decode_general_bound_is_the_measured_one():
    """The closeness bound of the general-logit GPU test: the largest error, in fp32 ulps of the float64 value, of torch's CPU fp32
    evaluation of the formula on the test's own inputs is DECODE_CPU_ULP per column group (not more, and not less than half), and
    the bound is twice that plus 2.  A decode with one anchor's width off by 1 % misses it by orders of magnitude."""
    worst = {k: 0.0 for k in ED.DECODE_GROUPS}
    for nb, ny, nx, nc, ldraw, row0, level in ED.DECODE_GENERAL:
        raw = ED.decode_general_case(nb, ny, nx, nc, ldraw)
        live = raw[:, :, :3 * (5 + nc)]
        assert float(live.abs().max()) == 100.0 and 0.01 < float((live.abs() > 8).float().mean()) < 0.06
        n = 3 * ny * nx
        ref = ED.decode_rule(torch.sigmoid(raw.double()), ny, nx, nc, 0, n, level, exact=False)
        got = ED.decode_f32_cpu(raw, ny, nx, nc, level)
        for k, cols in ED.DECODE_GROUPS.items():
            worst[k] = max(worst[k], ED.ulp_error(got[..., cols], ref[..., cols]))
        off = ref.clone()
        off[:, :ny * nx, 2] *= 1.01
        assert ED.ulp_error(off.float()[..., 2:4], ref[..., 2:4]) > 1000 * ED.DECODE_ULP_BOUND["wh"]
    for k in worst:
        assert worst[k] <= ED.DECODE_CPU_ULP[k] <= 2 * worst[k], (k, worst)
        assert ED.DECODE_ULP_BOUND[k] == 2 * ED.DECODE_CPU_ULP[k] + 2
    v = torch.tensor([1.0, 1.5, 2.0, 3.0e-39, 0.0, -6.0], dtype=torch.float64)
    assert ED.ulp32(v).tolist() == [2.0 ** -23, 2.0 ** -23, 2.0 ** -22, 2.0 ** -149, 2.0 ** -149, 2.0 ** -21]


# ------------------------------------------------------------------------------------------------ RootNet layout kernels
def test_gap_data_is_exact_and_sees_every_fault():
    """Every (B, HW, C) of the exact GPU test: the builder's bound holds (asserted inside gap_rule), and each fault changes more
    than half of the depths (all of them but one at B = 3); the batch faults apply where B > 1."""
    met = set()
    for B in ED.GAP_B:
        for HW in ED.GAP_HW:
            for C in ED.GAP_C:
                feat, w, bias, kv, depth = ED.gap_case(B, HW, C)
                assert len(set(kv.tolist())) == B and torch.equal(kv * 4, (kv * 4).round()) and bias == round(bias)
                for fault in ED.GAP_FAULTS:
                    if fault in ("k_value rotated", "image stride zero") and B == 1:
                        continue
                    got = ED.gap_rule(feat, w, bias, kv, fault=fault, exact=False)
                    changed = (got != depth)[1:] if fault == "image stride zero" else got != depth
                    assert float(changed.float().mean()) > HALF, (fault, B, HW, C)
                    met.add(fault)
    assert met == set(ED.GAP_FAULTS)
    with pytest.raises(AssertionError):
        ED.gap_rule(feat * 2.0 ** 12, w, bias, kv)


def test_layout_cases_are_what_the_issue_asks_for():
    assert [B * H * W for B, H, W in ED.NHWC8_SHAPES] == [1, 35, 816, 2046]
    for shape in ED.NHWC8_SHAPES:
        x = ED.nhwc8_case(*shape)
        assert float((x.reshape(-1)[1:] != x.reshape(-1)[:-1]).float().mean()) > HALF or x.numel() == 3
    for img_h, img_w, x0, win_w, patch, pad in ED.IM2COL_CASES:
        img = ED.im2col_case(3, img_h, img_w, x0, win_w, patch, pad)
        inside = img[..., x0:x0 + win_w]
        assert float(inside.abs().max()) < 2 and bool((img[..., :x0] == ED.IM2COL_OUTSIDE).all()) and bool((img[..., x0 + win_w:] == ED.IM2COL_OUTSIDE).all())
        ref = ED.im2col_rule(img, x0, win_w, patch, pad, torch.float32)
        gh, gw = (img_h + 2 * pad - patch) // patch + 1, (win_w + 2 * pad - patch) // patch + 1
        assert ref.shape == (3 * gh * gw, 3 * patch * patch) and float(ref.abs().max()) < 2
        assert (float((ref == 0).float().mean()) > 0) == (pad > 0)
    assert (256, 256, 32, 192, 16, 2) in ED.IM2COL_CASES and any(x0 + w == full and x0 > 0 for _, full, x0, w, _, _ in ED.IM2COL_CASES)


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


def test_fp8_epilogue_builder_refuses_a_residual_that_is_not_exact(monkeypatch):
    """fp8_case passes; the epilogue builder's own bound (bias and residual included) trips."""
    monkeypatch.setattr(ED, "FP8_RESID_RANGE", 1 << 24)
    ED.fp8_case(16, 64, 128, ED.FP8_EPILOGUE_WS_RANGE)
    with pytest.raises(AssertionError):
        ED.fp8_epilogue_case(16, 64, 128)


def test_attention_builder_refuses_a_gap_it_cannot_reach(monkeypatch):
    monkeypatch.setattr(ED, "ATT_GAP", 600.0)
    with pytest.raises(AssertionError):
        ED.attention_case(3, 4, 192, (1,))


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

