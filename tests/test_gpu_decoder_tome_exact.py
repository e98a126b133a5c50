"""hm_linear_f32 (csrc/decoder.hip) and the token-merging match / merge kernels (csrc/tome.hip) on exact data, bit for bit.

hm_linear_f32: hashed small-integer operands (tests/exact_data.py: every product and partial sum an integer below 2^24, so
exact on the fp32 MFMA in any order) at the shapes forward.hip launches and at a set of edge shapes that reach the row
clamps, the 4-column n >= N guard, waves without a K block and every way into and out of the 4-deep prefetch loop; as the
forward calls it: in place (the residual buffer is the output), with leading dimensions wider than the row.

Matching and merge: integer metric rows with integer norms, so every normalised value and cosine is a dyadic rational and
ties are plentiful and exact; the decisions (first maximum, stable descending rank, crowded dst tokens, r = Na) must be those
of tests/tome_rule.py, through hm_tome_merge_metric in three metric layouts and through hm_tome_merge in fp16 and bf16.
tests/test_exact_data_host.py shows on the CPU that this data tells each index or rule fault from the right answer.
"""
import functools
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exact_data as ED  # noqa: E402
import tome_rule as TR  # noqa: E402

from hamer_yolo_amd import ops

DEV = "cuda"
S_IN, S_OUT = 7.0, -12345.0           # what the columns beside X / W hold, and the sentinels around out / resid


# ------------------------------------------------------------------------------------------------ hm_linear_f32
@pytest.mark.parametrize("M,N,K", ED.LINEAR_F32_PROD + ED.LINEAR_F32_EDGE)
def test_linear_f32_exact_integers(M, N, K):
    """Bit-equal to torch with bias, without, with bias + residual, and with bias + residual in place (out is the residual
    buffer, as every residual launch of the decoder has it).  The output buffers start as NaN: an element left unwritten
    fails as well."""
    x, w, bias, resid = ED.gemm_case(M, N, K, resid=5)
    acc = x @ w.t()
    xd, wd, bd, rd = x.to(DEV), w.to(DEV), bias.to(DEV), resid.to(DEV)
    nan = lambda: torch.full((M, N), float("nan"), device=DEV)      # noqa: E731
    ED.assert_exact(ops.linear_f32(xd, wd, bd, out=nan()), acc + bias, (M, N, K, "bias"))
    ED.assert_exact(ops.linear_f32(xd, wd, out=nan()), acc, (M, N, K, "no bias"))
    ED.assert_exact(ops.linear_f32(xd, wd, bd, rd, out=nan()), acc + bias + resid, (M, N, K, "bias + residual"))
    assert torch.equal(rd.cpu(), resid)
    buf = rd.clone()
    assert ops.linear_f32(xd, wd, bd, buf, out=buf) is buf
    ED.assert_exact(buf, acc + bias + resid, (M, N, K, "bias + residual in place"))
    ED.assert_exact(ops.linear_f32(xd, wd, bd), acc + bias, (M, N, K, "bias, no out="))


def _slice(t, left, right, fill, spare_rows=0):
    """t (rows, cols) on the device as columns left .. left + cols of the first rows of a wider, longer buffer of `fill`."""
    buf = torch.full((t.shape[0] + spare_rows, left + t.shape[1] + right), fill, device=DEV)
    view = buf[:t.shape[0], left:left + t.shape[1]]
    view.copy_(t)
    return buf, view


def _around_untouched(buf, rows, left, cols, fill):
    return bool((buf[:, :left] == fill).all()) and bool((buf[:, left + cols:] == fill).all()) and bool((buf[rows:] == fill).all())


def _strided_operands(M, N, K):
    x, w, bias, resid = ED.gemm_case(M, N, K, resid=5)
    xb, xd = _slice(x, 4, 8, S_IN)
    wb, wd = _slice(w, 8, 12, S_IN)
    assert xd.stride(0) == K + 12 and wd.stride(0) == K + 20 and xd.data_ptr() % 16 == 0 and wd.data_ptr() % 16 == 0
    return x, w, bias, resid, xb, xd, wb, wd


@pytest.mark.parametrize("M,N,K", ED.LINEAR_F32_STRIDED)
def test_linear_f32_leading_dimensions_wider_than_the_row_exact(M, N, K):
    """ldx > K, ldw > K, ldo > N, ldr > N (multiples of 4, 16-byte aligned slices): X and W are column slices of wider buffers
    whose other columns hold a non-zero value (a K loop that runs past the row, or rows at the wrong pitch, change the sums);
    out and the residual sit between sentinel columns, with a spare sentinel row after row M - 1 (the row the clamp of a
    partial tile re-reads); every sentinel comes back untouched, out of place and in place.  One shape of whole tiles and one
    ragged in M, N and K."""
    x, w, bias, resid, xb, xd, wb, wd = _strided_operands(M, N, K)
    bd = bias.to(DEV)
    acc = x @ w.t()
    cb, cd = _slice(torch.full((M, N), S_OUT), 4, 8, S_OUT, spare_rows=1)
    rb, rd = _slice(resid, 8, 4, S_OUT, spare_rows=1)
    assert cd.stride(0) == N + 12 and rd.stride(0) == N + 12 and cd.data_ptr() % 16 == 0 and rd.data_ptr() % 16 == 0
    before = rb.clone()
    ops.linear_f32(xd, wd, bd, rd, out=cd)
    ED.assert_exact(cd, acc + bias + resid, (M, N, K, "strided, residual"))
    assert _around_untouched(cb, M, 4, N, S_OUT) and torch.equal(rb, before)
    ops.linear_f32(xd, wd, bd, rd, out=rd)
    ED.assert_exact(rd, acc + bias + resid, (M, N, K, "strided, residual in place"))
    assert _around_untouched(rb, M, 8, N, S_OUT)
    cb.fill_(S_OUT)
    ops.linear_f32(xd, wd, bd, out=cd)
    ED.assert_exact(cd, acc + bias, (M, N, K, "strided, bias"))
    assert _around_untouched(cb, M, 4, N, S_OUT)
    cb.fill_(S_OUT)
    ops.linear_f32(xd, wd, out=cd)
    ED.assert_exact(cd, acc, (M, N, K, "strided, no bias"))
    assert _around_untouched(cb, M, 4, N, S_OUT)
    assert _around_untouched(xb, M, 4, K, S_IN) and _around_untouched(wb, N, 8, K, S_IN)
    assert torch.equal(xd.cpu(), x) and torch.equal(wd.cpu(), w)


def test_linear_f32_gelu_strided_in_place():
    """act = 1 at the ragged strided shape with the residual in place: gelu(x W^T + b) + r against fp64 within the tolerance
    of test_linear_f32 (GELU is not exact; the sums going into it are), sentinels untouched."""
    M, N, K = ED.LINEAR_F32_STRIDED[1]
    x, w, bias, resid, xb, xd, wb, wd = _strided_operands(M, N, K)
    rb, rd = _slice(resid, 8, 4, S_OUT, spare_rows=1)
    ops.linear_f32(xd, wd, bias.to(DEV), rd, act=1, out=rd)
    ref = F.gelu(x.double() @ w.double().t() + bias.double()) + resid.double()
    np.testing.assert_allclose(rd.cpu().numpy(), ref.float().numpy(), atol=3e-6 * math.sqrt(K), rtol=1e-5)
    assert _around_untouched(rb, M, 8, N, S_OUT)


# ------------------------------------------------------------------------------------------------ matching and merge
@functools.lru_cache(maxsize=None)
def _tome_case(T, r):
    """The designed metric of the case, the rule's matching on it and, per D, (x, size, merged rows, merged sizes)."""
    metric = ED.tome_match_case(ED.TOME_B, T, ED.TOME_SALT.get(T, 0))
    idx = TR.match(metric, r)
    merged = {}
    for D in ED.TOME_D:
        x, size = ED.tome_merge_case(ED.TOME_B, T, D, ED.tome_sizes_given(T))
        merged[D] = (x, size) + TR.merge(x, size, *idx)
    return metric, idx, merged


def _assert_decisions(index, idx, T, r, what, prefill=None):
    """index (B, 3, 96) from the device: its three prefixes are the rule's unm | src | dst; with `prefill`, nothing else changed."""
    unm, src, dst = idx
    na = (T + 1) // 2
    got = index.cpu().long()
    assert got.shape == (ED.TOME_B, 3, 96)
    assert torch.equal(got[:, 1, :r], src), (what, "src", got[:, 1, :r].tolist(), src.tolist())
    assert torch.equal(got[:, 2, :r], dst), (what, "dst", got[:, 2, :r].tolist(), dst.tolist())
    assert torch.equal(got[:, 0, :na - r], unm), (what, "unm", got[:, 0, :na - r].tolist(), unm.tolist())
    if prefill is not None:
        rest = torch.ones_like(got, dtype=torch.bool)
        rest[:, 0, :na - r] = False
        rest[:, 1:, :r] = False
        assert bool((got[rest] == prefill).all()), (what, "index workspace written outside its three prefixes")


def _assert_merged(xo, so, x_ref, s_ref, what):
    """x_out / size_out with one spare sentinel row each: rows bit-equal to the rule, the sentinel rows untouched."""
    rows, D = x_ref.shape[0] * x_ref.shape[1], x_ref.shape[2]
    ED.assert_exact(so[:rows], s_ref.reshape(rows), what + ("size_out",))
    ED.assert_exact(xo[:rows], x_ref.reshape(rows, D), what + ("x_out",))
    assert bool((xo[rows:] == S_OUT).all()) and bool((so[rows:] == S_OUT).all()), what + ("sentinel row",)


@pytest.mark.parametrize("layout", ED.TOME_LAYOUTS)
@pytest.mark.parametrize("T,r", ED.TOME_EXACT)
def test_tome_merge_metric_exact(T, r, layout):
    """hm_tome_merge_metric (the entry HamerEngine(token_merge=...) uses) on the exact matching data, the metric handed over
    as contiguous rows, as 80 columns inside rows of 96 with a non-zero fill around them, and as hi + lo parts 88 columns
    apart in rows of 176: unm, src and dst are the rule's, an index workspace prefilled with -1 has changed in its three
    prefixes per crop only, size_out and x_out (D = 8 and 320, sizes given except at T = 192) equal the rule bit for bit --
    both divide the same exact integers in fp32 -- and their spare rows are untouched."""
    B = ED.TOME_B
    metric, idx, merged = _tome_case(T, r)
    buf, first, cols, lo_off = ED.tome_metric_layout(metric, layout)
    view = buf.to(DEV)[:, first:first + cols]
    assert view.stride(0) == {"ld80": 80, "ld96": 96, "hi_lo": 176}[layout]
    for D in ED.TOME_D:
        x, size, x_ref, s_ref = merged[D]
        rows = B * (T - r)
        xo = torch.full((rows + 1, D), S_OUT, device=DEV)
        so = torch.full((rows + 1,), S_OUT, device=DEV)
        index = torch.full((B * 3 * 96,), -1, device=DEV, dtype=torch.int32)
        sd = size.reshape(B * T).to(DEV) if size is not None else None
        _, _, got = ops.tome_merge_metric(view, lo_off, x.reshape(B * T, D).to(DEV), sd, B, T, r, x_out=xo, size_out=so, index=index)
        what = (T, r, layout, D)
        _assert_decisions(got, idx, T, r, what, prefill=-1)
        _assert_merged(xo, so, x_ref, s_ref, what)


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("T,r", ED.TOME_EXACT)
def test_tome_merge_from_keys_exact(T, r, dt):
    """hm_tome_merge with four heads of 16-bit keys metric + delta_h, the delta_h hashed integers that sum to zero over the
    heads (all values exact in bf16): the metric workspace is the designed metric bit for bit, and the decisions and merged
    rows are the rule's."""
    B, heads = ED.TOME_B, 4
    metric, idx, merged = _tome_case(T, r)
    qkv = ED.tome_head_keys(metric, heads, dt).to(DEV)
    for D in ED.TOME_D:
        x, size, x_ref, s_ref = merged[D]
        sd = size.reshape(B * T).to(DEV) if size is not None else None
        xo, so, index, mws = ops.tome_merge(qkv, x.reshape(B * T, D).to(DEV), sd, B, T, r, heads, ED.TOME_HD)
        what = (T, r, dt, D)
        ED.assert_exact(mws.reshape(B * T, ED.TOME_HD), metric.reshape(B * T, ED.TOME_HD), what + ("metric workspace",))
        _assert_decisions(index, idx, T, r, what)
        ED.assert_exact(so, s_ref.reshape(-1), what + ("size_out",))
        ED.assert_exact(xo, x_ref.reshape(-1, D), what + ("x_out",))
