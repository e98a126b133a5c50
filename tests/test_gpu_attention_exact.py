"""The attention kernels on data whose softmax is exactly few-hot (tests/exact_data.py, section "attention").

Every (crop, head) has a code book: keys of a group share a sign code, a query carries the code of the group of the one key it
was dealt, the top logits are all exactly 640 in the log2 domain and every other key lies at least 160 below, where an fp32
exponential is exactly zero.  P is then 1 on the m keys of the group (m in 1, 2, 4), the row sum m, and the accumulator the
integer-valued sum of the group's V rows: the 16-bit output is ONE rounding of an exactly known number, the MXFP8 output the
oracle quantiser of the exact fp32 rows, the fp32 output the number itself.  All comparisons are torch.equal on the bits.  The
key permutation of the P^T slots, the transposing V reads, the double buffer and its counted waits, the 96-column MXFP8 pad and
its scale layout are index maps; tests/test_exact_data_host.py shows that this data sees a fault in each of them.

vit_attention_kernel runs dense (bf16, fp16), with MXFP8 output and with token merging, each at the device's grid and under the
HM_OPT_ATT_GRID settings of tests/test_gpu_attention_items.py (one item per workgroup, several, a ragged last round), so both
halves of the double buffer compute hashed items.  Outputs go into sentinel-filled buffers with guard rows.
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exact_data as ED  # noqa: E402
import test_gpu_attention_items as AI  # noqa: E402

from hamer_yolo_amd import lib as L
from hamer_yolo_amd import ops

DEV = "cuda"
T, HD, HDP, GUARD = ED.ATT_T, ED.ATT_HD, ED.ATT_HDP, AI.GUARD
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
TOME_OPTIONS = (0, 3)                              # 12 items: one per workgroup, and 4 per workgroup on 3


@functools.lru_cache(maxsize=None)
def _case(B, heads, tokens, gs, sizes=None):
    """Built once per case and left unchanged."""
    return ED.attention_case(B, heads, tokens, gs, sizes)


def _bits16(t):
    return t.contiguous().view(torch.int16)


def _launch16(kind, qkv, size, B, heads, Tn, scale):
    """One launch of the dense or the token-merging kernel into a sentinel-filled buffer with guard rows; the int16 bits."""
    rows = B * Tn
    buf = torch.full((rows + GUARD, heads * HD), -1, dtype=torch.int16, device=DEV).view(qkv.dtype)
    if kind == "tome":
        assert ops.tome_attention(qkv, size, B, Tn, heads, HD, scale, out=buf) is buf
    else:
        assert ops.vit_attention(qkv, B, Tn, heads, HD, scale, out=buf) is buf
    bits = buf.view(torch.int16)
    assert bool((bits[rows:] == -1).all()), "guard rows overwritten"
    return bits[:rows].cpu()


def _launch_mx8(qkv, B, heads, scale):
    rows = B * T
    out8 = torch.full((rows + GUARD, heads * HDP), 0xFF, dtype=torch.uint8, device=DEV)
    flat = torch.full((heads * 3 * rows + 256,), 0xFF, dtype=torch.uint8, device=DEV)
    scales = flat[:heads * 3 * rows].view(heads * 3, rows)
    ops.vit_attention_mx8(qkv, B, T, heads, HD, scale, out8=out8, scales=scales)
    assert bool((out8[rows:] == 0xFF).all()) and bool((flat[heads * 3 * rows:] == 0xFF).all()), "guard bytes overwritten"
    return out8[:rows].cpu(), scales.cpu()


def _geometries(items):
    """(option, per, grid) of every setting, from the library's own arithmetic; the set must hold one item per workgroup,
    two and more than two (both halves of the double buffer, a buffer re-used)."""
    geo = [(o,) + AI._geometry(items, o) for o in AI.OPTIONS]
    assert any(per == 1 for _, per, _ in geo) and any(per == 2 for _, per, _ in geo) and any(per >= 3 for _, per, _ in geo)
    return geo


def test_settings_reach_a_ragged_last_round():
    """Over the dense shapes, the settings hold a launch whose last round is ragged (the 12 items of 3 x 4 divide evenly under
    every setting; the 32 of 2 x 16 do not)."""
    assert any(per >= 2 and B * heads % grid for B, heads, _ in ED.ATT_DENSE for _, per, grid in _geometries(B * heads))


def test_the_dense_scale_gives_two_to_the_minus_three():
    """launch_att multiplies the scale by 1.44269504088896340736f in fp32: with ED.ATT_SCALE_DENSE the product is exactly 2^-3."""
    assert np.float32(ED.ATT_SCALE_DENSE) * ED.ATT_LOG2E == np.float32(2.0 ** -3)


@pytest.mark.parametrize("B,heads,gs", ED.ATT_DENSE, ids=[f"{B}x{h}-{'few' if len(g) > 1 else 'one'}hot" for B, h, g in ED.ATT_DENSE])
@pytest.mark.parametrize("variant", ["bf16", "fp16", "mx8"])
def test_dense_and_mx8_exact(variant, B, heads, gs):
    """Dense bf16 / fp16: the exact result rounded once.  MXFP8: every byte and every scale of the oracle quantiser on the exact
    fp32 rows widened to 96 columns per head, the 16 pad columns zero bytes.  At every HM_OPT_ATT_GRID setting."""
    c = _case(B, heads, T, gs)
    dt = torch.bfloat16 if variant == "mx8" else DTYPES[variant]
    qkv = c["qkv"].to(dt).to(DEV)
    if variant == "mx8":
        exp8, exps = ED.att_mx8_expect(c["expect"], heads)
    else:
        expect = _bits16(c["expect"].float().to(dt))
    for option, per, grid in _geometries(B * heads):
        print(f"{variant} B={B} heads={heads} groups={gs}: option={option} per={per} grid={grid} gap={c['gap']}")
        with L.option(L.HM_OPT_ATT_GRID, option):
            if variant == "mx8":
                o8, os_ = _launch_mx8(qkv, B, heads, ED.ATT_SCALE_DENSE)
                ED.assert_exact(os_, exps, f"mx8 scales, option {option}")
                ED.assert_exact(o8, exp8, f"mx8 bytes, option {option}")
                assert bool((o8.reshape(B * T, heads, HDP)[:, :, HD:] == 0).all())
            else:
                ED.assert_exact(_launch16("dense", qkv, None, B, heads, T, ED.ATT_SCALE_DENSE), expect, f"{variant}, option {option}")


@pytest.mark.parametrize("variant", ["bf16", "fp16"])
def test_dominant_key_at_the_production_scale(variant):
    """scale = 80^-0.5: fma(m, c, -(m c)) is only the rounding residual of m c, p = exp2(residual) is within 1e-5 of 1 and the
    output v / p rounds back to v (ED.att_production_margin emulates both roundings on the CPU and asserts the margin)."""
    B, heads, gs = ED.ATT_PRODUCTION
    c, dt = _case(B, heads, T, gs), DTYPES[variant]
    coef, res, delta = ED.att_production_margin(c, HD ** -0.5, dt)
    print(f"{variant}: c = {coef!r}, residual {res:.3e}, |p - 1| <= {delta:.3e}")
    expect = _bits16(c["expect"].float().to(dt))
    for option in (0, 3):
        with L.option(L.HM_OPT_ATT_GRID, option):
            ED.assert_exact(_launch16("dense", c["qkv"].to(dt).to(DEV), None, B, heads, T, HD ** -0.5), expect, f"{variant}, option {option}")


@pytest.mark.parametrize("variant", ["bf16", "fp16"])
def test_tome_exact_at_every_token_count(variant):
    """hm_tome_attention at every token count of the merging schedule and the edges 1, 15, 16, 17, 191, 192: dominant-key data
    with size = None and with hashed sizes 1..8 (a shift of at most 3 in the log2 domain, the gap stays >= 160: the same exact
    rows), few-hot data with size = None.  The dominant-key cases also run on the fp32 lane-per-key kernel
    (HM_OPT_TOME_SCALAR_ATTENTION), which must give the same rows.  Key 0 and key tokens - 1 are chosen keys in every case
    (every key is: asserted by the builder)."""
    B, heads, dt = ED.ATT_TOME_B, ED.ATT_TOME_HEADS, DTYPES[variant]
    assert set(ED.att_tome_tokens()) >= {1, 15, 16, 17, 191, 192, 176, 161, 23}
    for Tn in ED.att_tome_tokens():
        for gs, sizes in (((1,), None), ((1,), "hashed"), ((1, 2, 4), None)):
            c = _case(B, heads, Tn, gs, sizes)
            qkv = c["qkv"].to(dt).to(DEV)
            size = None if c["size"] is None else c["size"].to(DEV)
            expect = _bits16(c["expect"].float().to(dt))
            for option in TOME_OPTIONS:
                with L.option(L.HM_OPT_ATT_GRID, option):
                    ED.assert_exact(_launch16("tome", qkv, size, B, heads, Tn, ED.ATT_SCALE_DENSE), expect,
                                    f"{variant} tokens={Tn} groups={gs} sizes={sizes} option={option}")
            if gs == (1,):
                with L.option(L.HM_OPT_TOME_SCALAR_ATTENTION, 1):
                    ED.assert_exact(_launch16("tome", qkv, size, B, heads, Tn, ED.ATT_SCALE_DENSE), expect,
                                    f"{variant} scalar kernel tokens={Tn} sizes={sizes}")


@pytest.mark.parametrize("variant", ["bf16", "fp16"])
def test_tome_sizes_decide(variant):
    """Groups of three identical keys with sizes 1, 1, 2: the weights are 1/4, 1/4, 1/2.  This rests on v_log_f32 returning k
    exactly at 2^k (here 0 at 1 and 1 at 2), an assumption no earlier test of this project had measured.  It holds on the
    MI355X: the rows are bit-equal in both types at both grids (had it not, the comparison would have been the float64
    closed form at rtol = 2^-20).  The distance to the unrounded closed form is printed."""
    B, heads, dt = ED.ATT_TOME_B, ED.ATT_TOME_HEADS, DTYPES[variant]
    c = _case(B, heads, ED.ATT_TOME_DECIDES, (3,), "decides")
    expect = c["expect"].float().to(dt)
    for option in TOME_OPTIONS:
        with L.option(L.HM_OPT_ATT_GRID, option):
            got = _launch16("tome", c["qkv"].to(dt).to(DEV), c["size"].to(DEV), B, heads, ED.ATT_TOME_DECIDES, ED.ATT_SCALE_DENSE)
        d = (got.view(dt).double() - c["expect"]).abs()
        print(f"{variant} option {option}: max |out - closed form| {float(d.max()):.3e} "
              f"(relative {float((d / c['expect'].abs().clamp(min=0.25)).max()):.3e}), bits equal: {torch.equal(got, _bits16(expect))}")
        ED.assert_exact(got, _bits16(expect), f"{variant} sizes decide, option {option}")


@pytest.mark.parametrize("B,heads,gs", ED.ATT_F32, ids=[f"{B}x{h}-{'few' if len(g) > 1 else 'one'}hot" for B, h, g in ED.ATT_F32])
def test_attention_f32_exact(B, heads, gs):
    """hm_vit_attention_f32 (q scaled by 2^-3 first, expf, IEEE division): the exact fp32 value, no rounding involved."""
    c = _case(B, heads, T, gs)
    out = ops.vit_attention_f32(c["qkv"].to(DEV), B, T, heads, HD, ED.ATT_SCALE_F32)
    ED.assert_exact(out.cpu().double(), c["expect"], f"f32 B={B} heads={heads} groups={gs}")
