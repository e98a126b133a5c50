"""The persistent attention kernel (csrc/attention.hip) with several (crop, head) items per workgroup.

A workgroup walks its items at stride gridDim.x: K and V of item i+1 arrive by hand-counted LDS-DMA in the other half of a
double buffer while item i is computed, the next item's Q (and, with token merging, log2(size)) travels in a second register
set, and items are dealt through xcd_remap.  launch_att gives every workgroup ceil(items / CUs) items, so on a 256-CU chip
nothing below 257 items reaches the second step of that loop.  HM_OPT_ATT_GRID replaces the CU count; these tests use it to
run all five instantiations (dense bf16 / fp16, MXFP8 output, token merging bf16 / fp16) with 2 to 48 items per workgroup.

Principle: an item's arithmetic does not depend on which workgroup, buffer or step computes it, so any launch must equal BIT
FOR BIT the launches in which every workgroup has one item (the "reference launch": chunks of whole crops with
chunk * heads <= CUs at option 0).  The reference launch itself is pinned to a float64 statement on the CPU at one
multi-item setting per instantiation, so both cannot be wrong in the same way.

Every launch writes into a caller-provided buffer filled with a sentinel the kernel cannot produce (0xFFFF, a NaN, for the
16-bit outputs; 0xFF, the NaN of e4m3 and of E8M0, for the MXFP8 bytes and scales) with guard rows behind it: a caching
allocator cannot hand a correct earlier result back, and rows a launch never writes show.  Geometry is asserted from
hm_attention_grid (the function launch_att itself calls), never assumed.
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from hamer_yolo_amd import lib as L
from hamer_yolo_amd import ops, synth
from oracle import fp8_ref as Q

DEV = "cuda"
T, HD, HDP = 192, 80, 96
SCALE = HD ** -0.5
GUARD = 8                                        # sentinel rows behind every output
VARIANTS = ("bf16", "fp16", "mx8", "tome_bf16", "tome_fp16")
SHAPES = ((5, 4), (3, 16))                       # (B, heads): 20 and 48 items
OPTIONS = (0, 1, 3, 8, 12, 16)                   # HM_OPT_ATT_GRID; 0 is the control
# token merging: (tokens per crop, size given).  The last wave with a query is wave 0 (1, 3, 16), 1 (23), 10 (161) and 11
# (192); 192 ends K and V on whole 64-chunk copy groups, the others on partial ones; below 177 tokens some waves have no query
TOME_CASES = ((192, True), (161, True), (23, True), (16, True), (3, True), (1, True), (161, False))


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _dtype(variant):
    return torch.float16 if variant.endswith("fp16") else torch.bfloat16


def _ulp16(dtype):
    return 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -11


def _geometry(items, option, cus=None):
    """(per, grid) of a launch of `items` items under HM_OPT_ATT_GRID = option, from the library's own arithmetic."""
    with L.option(L.HM_OPT_ATT_GRID, option):
        grid = L.load().hm_attention_grid(items, cus or _cus())
    assert 1 <= grid <= items
    return -(-items // grid), grid


def _xcd_remap(bid, nwg):
    """common.h xcd_remap: workgroup `bid` of `nwg` starts at this item."""
    xcd, q, r = bid & 7, nwg >> 3, nwg & 7
    return (xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q) + (bid >> 3)


# ------------------------------------------------------------------------------------ operands
@functools.lru_cache(maxsize=None)
def _operands(variant, B, heads, Tn, with_size):
    """(qkv, size) on the device, with the half-widths of the existing kernel tests: 2.0 dense, 1.5 MX8, 1.2 token merging."""
    if variant.startswith("tome"):
        qkv = synth.uniform("tq", (B * Tn, 3 * heads * HD), 1.2, seed=Tn).to(_dtype(variant))
        # hashed per token of the whole batch: every crop has its own sizes
        size = (1.0 + (synth._hash_u32(torch.arange(B * Tn, dtype=torch.int64), 7) % 4).float()) if with_size else None
        return qkv.to(DEV), (size.to(DEV) if with_size else None)
    if variant == "mx8":
        return synth.uniform("aq", (B * T, 3 * heads * HD), 1.5, seed=11).to(torch.bfloat16).to(DEV), None
    return synth.uniform("qkv", (B * T, 3 * heads * HD), 2.0, seed=heads).to(_dtype(variant)).to(DEV), None


# ------------------------------------------------------------------------------------ launches into sentinel-filled buffers
def _launch(variant, qkv, size, B, heads, Tn):
    """One launch.  Returns the raw bits written: (int16 (B*Tn, heads*80),) or (uint8 (B*192, heads*96), uint8 (heads*3,
    B*192)) for MX8 -- views of the sentinel-filled buffers, whose guard rows are checked here."""
    rows = B * Tn
    if variant == "mx8":
        out8 = torch.full((rows + GUARD, heads * HDP), 0xFF, dtype=torch.uint8, device=DEV)
        flat = torch.full((heads * 3 * rows + 256,), 0xFF, dtype=torch.uint8, device=DEV)
        scales = flat[:heads * 3 * rows].view(heads * 3, rows)
        ops.vit_attention_mx8(qkv, B, T, heads, HD, SCALE, out8=out8, scales=scales)
        assert bool((out8[rows:] == 0xFF).all()) and bool((flat[heads * 3 * rows:] == 0xFF).all()), "guard bytes overwritten"
        return out8[:rows], scales
    buf = torch.full((rows + GUARD, heads * HD), -1, dtype=torch.int16, device=DEV).view(qkv.dtype)
    if variant.startswith("tome"):
        assert ops.tome_attention(qkv, size, B, Tn, heads, HD, SCALE, out=buf) is buf
    else:
        assert ops.vit_attention(qkv, B, T, heads, HD, SCALE, out=buf) is buf
    bits = buf.view(torch.int16)
    assert bool((bits[rows:] == -1).all()), "guard rows overwritten"
    return (bits[:rows],)


def _reference_launch(variant, qkv, size, B, heads, Tn):
    """The same inputs in chunks of whole crops, one item per workgroup (asserted), option 0; chunk outputs concatenated."""
    cus = _cus()
    chunk = cus // heads
    assert chunk >= 1
    parts = []
    with L.option(L.HM_OPT_ATT_GRID, 0):
        for b0 in range(0, B, chunk):
            n = min(chunk, B - b0)
            assert L.load().hm_attention_grid(n * heads, cus) == n * heads
            parts.append(_launch(variant, qkv[b0 * Tn:(b0 + n) * Tn], None if size is None else size[b0 * Tn:(b0 + n) * Tn],
                                 n, heads, Tn))
    ref = (torch.cat([p[0] for p in parts], 0),)
    if variant == "mx8":
        ref += (torch.cat([p[1] for p in parts], 1),)       # scales are [heads*3][rows]
    for r in ref:                                            # every element written: no sentinel left
        assert not bool((r == (0xFF if r.dtype == torch.uint8 else -1)).any()), "the reference launch left sentinel values"
    return ref


@functools.lru_cache(maxsize=None)
def _reference(variant, B, heads, Tn, with_size):
    """Computed once per case and kept alive (and unchanged) for every test that compares against it."""
    qkv, size = _operands(variant, B, heads, Tn, with_size)
    return _reference_launch(variant, qkv, size, B, heads, Tn)


# ------------------------------------------------------------------------------------ bit identity, with a report per item
def _item_report(got, ref, B, heads, Tn, grid, what):
    """None when the launch equals the reference bit for bit; else, per differing item: its workgroup, step and buffer in
    the item loop and the first differing row and column inside the item."""
    if all(torch.equal(g, r) for g, r in zip(got, ref)):
        return None
    start = {_xcd_remap(bid, grid): bid for bid in range(grid)}
    assert sorted(start) == list(range(grid))
    lines = []
    for item in range(B * heads):
        b, h = divmod(item, heads)
        for k, (g, r) in enumerate(zip(got, ref)):
            if k == 0:                                        # rows of the crop, the head's columns
                w = g.shape[1] // heads
                gi, ri = g[b * Tn:(b + 1) * Tn, h * w:(h + 1) * w], r[b * Tn:(b + 1) * Tn, h * w:(h + 1) * w]
            else:                                             # MX8 scales: the head's 3 blocks, the crop's rows
                gi, ri = g[h * 3:h * 3 + 3, b * Tn:(b + 1) * Tn].t(), r[h * 3:h * 3 + 3, b * Tn:(b + 1) * Tn].t()
            bad = (gi != ri).nonzero()
            if bad.numel():
                r0, c0 = (int(x) for x in bad[0])
                step = item // grid
                lines.append(f"item {item} (crop {b}, head {h}; workgroup {start[item % grid]}, step {step}, buffer {step & 1})"
                             f"{' scales' if k else ''}: {bad.shape[0]} of {gi.numel()} wrong, first at (row {r0}, col {c0}): "
                             f"got {int(gi[r0, c0]) & 0xFFFF:#06x}, expected {int(ri[r0, c0]) & 0xFFFF:#06x}")
    return f"{what}: {len(lines)} item entries differ from one-item-per-workgroup launches\n" + "\n".join(lines[:40])


def _assert_items_identical(variant, B, heads, Tn, with_size, option, require_multi=True):
    items = B * heads
    per, grid = _geometry(items, option)
    print(f"{variant} Tn={Tn} size={'hashed' if with_size else None}: items={items} option={option} per={per} grid={grid}")
    if option and require_multi:
        assert per >= 2, "this setting does not give a workgroup a second item"
    qkv, size = _operands(variant, B, heads, Tn, with_size)
    ref = _reference(variant, B, heads, Tn, with_size)
    with L.option(L.HM_OPT_ATT_GRID, option):
        for rep in range(2):                                  # twice, into freshly sentinel-filled buffers
            got = _launch(variant, qkv, size, B, heads, Tn)
            msg = _item_report(got, ref, B, heads, Tn, grid, f"{variant} B={B} heads={heads} Tn={Tn} option={option} run {rep}")
            assert msg is None, msg


def test_settings_reach_every_path_of_the_item_loop():
    """The (items, option) pairs below must include, by the library's own arithmetic: one workgroup walking everything; an
    odd number of items per workgroup (the loop leaves through the break inside the unrolled pair) and an even one (it leaves
    through the loop condition); a ragged last round; a grid above 8 that is no multiple of 8 (the remainder branch of
    xcd_remap) and one that is (a non-identity permutation); more than two items, so a buffer is re-used."""
    geo = {(B * heads, o): _geometry(B * heads, o) for B, heads in SHAPES for o in OPTIONS if o}
    for (items, o), (per, grid) in geo.items():
        print(f"items={items} option={o} per={per} grid={grid}")
        assert per >= 2 and grid == -(-items // per)
    assert any(grid == 1 for per, grid in geo.values())
    assert any(per % 2 == 1 and items % grid == 0 for (items, o), (per, grid) in geo.items())     # every workgroup: odd count
    assert any(per % 2 == 0 and items % grid == 0 for (items, o), (per, grid) in geo.items())     # every workgroup: even count
    assert any(items % grid != 0 for (items, o), (per, grid) in geo.items())
    assert geo[(20, 12)] == (2, 10)
    assert any(grid > 8 and grid % 8 != 0 for per, grid in geo.values())
    multiples = [grid for per, grid in geo.values() if grid > 8 and grid % 8 == 0]
    assert multiples and any(_xcd_remap(b, g) != b for g in multiples for b in range(g))
    assert geo[(48, 16)] == (3, 16)
    assert any(per >= 3 for per, grid in geo.values())
    # token merging: first, a middle and the last wave hold the last query; whole and partial last copy groups
    last_wave = {(Tn - 1) // 16 for Tn, _ in TOME_CASES}
    assert 0 in last_wave and 11 in last_wave and any(0 < w < 11 for w in last_wave)
    assert any(Tn * 11 % 64 == 0 and Tn * 10 % 64 == 0 for Tn, _ in TOME_CASES)
    assert any(Tn * 11 % 64 and Tn * 10 % 64 for Tn, _ in TOME_CASES)
    assert any(not s for _, s in TOME_CASES)


@pytest.mark.parametrize("option", OPTIONS)
@pytest.mark.parametrize("B,heads", SHAPES)
@pytest.mark.parametrize("variant", VARIANTS[:3])
def test_dense_and_mx8_items_per_workgroup_bit_identical(variant, B, heads, option):
    _assert_items_identical(variant, B, heads, T, False, option)


@pytest.mark.parametrize("option", OPTIONS)
@pytest.mark.parametrize("B,heads", SHAPES)
@pytest.mark.parametrize("variant", VARIANTS[3:])
def test_tome_items_per_workgroup_bit_identical(variant, B, heads, option):
    """Token merging adds per-buffer state: log2(size) staged per buffer, V rows past Tn zeroed once per launch and relied
    on afterwards, copies and waves that stop at Tn."""
    for Tn, with_size in TOME_CASES:
        _assert_items_identical(variant, B, heads, Tn, with_size, option)


# ------------------------------------------------------------------------------------ accuracy at a multi-item setting
ACC_B, ACC_HEADS, ACC_OPTION = 5, 4, 3            # 20 items on 3 workgroups: 7 + 7 + 6


def _acc_launch(variant, Tn=T, with_size=False):
    per, grid = _geometry(ACC_B * ACC_HEADS, ACC_OPTION)
    assert (per, grid) == (7, 3)
    print(f"{variant} Tn={Tn}: items={ACC_B * ACC_HEADS} option={ACC_OPTION} per={per} grid={grid}")
    qkv, size = _operands(variant, ACC_B, ACC_HEADS, Tn, with_size)
    with L.option(L.HM_OPT_ATT_GRID, ACC_OPTION):
        got = _launch(variant, qkv, size, ACC_B, ACC_HEADS, Tn)
    return qkv.cpu(), (None if size is None else size.cpu()), got


def _f64_attention(qkv, size, B, heads, Tn, p_dtype=None):
    """softmax(scale q k^T + log(size)) v in float64, (B*Tn, heads*80); p_dtype: P = exp(s - max) rounded to the operand
    type before the product with V and divided by its unrounded row sum, as the dense kernel does."""
    q, k, v = qkv.double().reshape(B, Tn, 3, heads, HD).permute(2, 0, 3, 1, 4)
    s = (q @ k.transpose(-2, -1)) * SCALE
    if size is not None:
        s = s + size.double().reshape(B, 1, 1, Tn).log()
    if p_dtype is None:
        o = s.softmax(-1) @ v
    else:
        p = torch.exp(s - s.amax(-1, keepdim=True))
        o = (p.to(p_dtype).double() @ v) / p.sum(-1, keepdim=True)
    return o.transpose(1, 2).reshape(B * Tn, heads * HD)


@pytest.mark.parametrize("variant", ["bf16", "fp16"])
def test_dense_accuracy_with_seven_items_per_workgroup(variant):
    """The two statements of test_vit_attention with their tolerances, in float64."""
    dt = _dtype(variant)
    qkv, _, (bits,) = _acc_launch(variant)
    out = bits.view(dt).cpu().double()
    assert torch.isfinite(out).all()
    ref = _f64_attention(qkv, None, ACC_B, ACC_HEADS, T, p_dtype=dt)
    exact = _f64_attention(qkv, None, ACC_B, ACC_HEADS, T)
    print(f"{variant}: max |out - rounded-P statement| {float((out - ref).abs().max()):.3e}, "
          f"max |out - exact softmax| {float((out - exact).abs().max()):.3e}")
    np.testing.assert_allclose(out.numpy(), ref.numpy(), atol=2e-3 if dt == torch.bfloat16 else 3e-4, rtol=2 * _ulp16(dt))
    np.testing.assert_allclose(out.numpy(), exact.numpy(), atol=1.5e-2 if dt == torch.bfloat16 else 2e-3, rtol=0)


def test_mx8_accuracy_with_seven_items_per_workgroup():
    """The statement of test_vit_attention_mx8_matches_16bit_kernel_then_quantised: dequantised, the output is within
    blockmax * 2^-3 + 1e-6 of the bf16 kernel's output (taken at the same setting, and itself held to the exact softmax
    here); pad columns are exact zeros."""
    B, H = ACC_B, ACC_HEADS
    qkv, _, (o8, os_) = _acc_launch("mx8")
    buf = torch.full((B * T + GUARD, H * HD), -1, dtype=torch.int16, device=DEV).view(torch.bfloat16)
    with L.option(L.HM_OPT_ATT_GRID, ACC_OPTION):
        ops.vit_attention(qkv.to(DEV), B, T, H, HD, SCALE, out=buf)
    ref16 = buf[:B * T].float().cpu()
    exact = _f64_attention(qkv, None, B, H, T)
    np.testing.assert_allclose(ref16.double().numpy(), exact.numpy(), atol=1.5e-2, rtol=0)
    o8, os_ = o8.cpu(), os_.cpu()
    deq = Q.mx8_dequantize(o8, os_).reshape(B * T, H, HDP)
    assert (deq[:, :, HD:] == 0).all() and (o8.reshape(B * T, H, HDP)[:, :, HD:] == 0).all()
    got = deq[:, :, :HD].reshape(B * T, H * HD)
    blockmax = torch.zeros(B * T, H, HDP)
    blockmax[:, :, :HD] = ref16.reshape(B * T, H, HD).abs()
    blockmax = blockmax.reshape(B * T, H * 3, 32).amax(-1, keepdim=True).expand(-1, -1, 32).reshape(B * T, H, HDP)[:, :, :HD]
    blockmax = blockmax.reshape(B * T, H * HD)
    err = (got - ref16).abs()
    print(f"mx8: max |dequantised - bf16 kernel| {float(err.max()):.3e}, largest share of its bound "
          f"{float((err / (blockmax * 2.0 ** -3 + 1e-6)).max()):.3f}")
    assert (err <= blockmax * 2.0 ** -3 + 1e-6).all()


@pytest.mark.parametrize("variant", ["tome_bf16", "tome_fp16"])
def test_tome_accuracy_with_seven_items_per_workgroup(variant):
    """fp16: the statement and tolerance of test_tome_kernels_vs_oracle (atol = rtol = 2e-3).  bf16: rtol = 2 ulp16(bf16),
    atol = 2e-3, the dense bf16 bounds -- the token-merging kernel carries P as hi + lo parts, so it is at least as exact as
    the dense kernel and the dense bound is an upper bound.  The fp32 lane-per-key kernel (HM_OPT_TOME_SCALAR_ATTENTION), a
    second opinion on the same inputs, must meet the same bound."""
    dt = _dtype(variant)
    atol, rtol = (2e-3, 2e-3) if dt == torch.float16 else (2e-3, 2 * _ulp16(dt))
    for Tn, with_size in TOME_CASES:
        qkv, size, (bits,) = _acc_launch(variant, Tn, with_size)
        ref = _f64_attention(qkv, size, ACC_B, ACC_HEADS, Tn)
        out = bits.view(dt).cpu().double()
        with L.option(L.HM_OPT_TOME_SCALAR_ATTENTION, 1):
            qd, sd = _operands(variant, ACC_B, ACC_HEADS, Tn, with_size)
            scalar = _launch(variant, qd, sd, ACC_B, ACC_HEADS, Tn)[0].view(dt).cpu().double()
        for name, o in (("MFMA kernel", out), ("scalar kernel", scalar)):
            assert torch.isfinite(o).all(), (name, Tn)
            d = (o - ref).abs()
            print(f"{variant} Tn={Tn} {name}: max abs err {float(d.max()):.3e}, largest share of atol + rtol |ref| "
                  f"{float((d / (atol + rtol * ref.abs())).max()):.3f}")
            np.testing.assert_allclose(o.numpy(), ref.numpy(), atol=atol, rtol=rtol, err_msg=f"{name}, {Tn} tokens")


# ------------------------------------------------------------------------------------ the device's own grid
@pytest.mark.parametrize("variant,Tn", [("fp16", T), ("tome_fp16", 161)])
def test_device_grid_with_a_ragged_third_round_bit_identical(variant, Tn):
    """Option 0 at a batch that gives this device more than two items per workgroup and a ragged last round (256 CUs: 40
    crops x 16 heads = 640 items, 3 per workgroup, grid 214).  Bit identity against chunked launches only."""
    heads, cus = 16, _cus()
    B = (5 * cus) // (2 * heads)
    while True:
        per, grid = _geometry(B * heads, 0)
        if B * heads > 2 * cus and (B * heads) % grid != 0:
            break
        B += 1
    items = B * heads
    print(f"{variant} Tn={Tn}: items={items} option=0 per={per} grid={grid} (CUs {cus}, B {B})")
    assert per >= 3
    if variant.startswith("tome"):
        qkv = synth.uniform("tq", (B * Tn, 3 * heads * HD), 1.2, seed=Tn, device=DEV).half()
        size = 1.0 + (synth._hash_u32(torch.arange(B * Tn, dtype=torch.int64, device=DEV), 7) % 4).float()
    else:
        qkv, size = synth.uniform("qkv", (B * Tn, 3 * heads * HD), 2.0, seed=heads, device=DEV).half(), None
    ref = _reference_launch(variant, qkv, size, B, heads, Tn)
    with L.option(L.HM_OPT_ATT_GRID, 0):
        for rep in range(2):
            got = _launch(variant, qkv, size, B, heads, Tn)
            msg = _item_report(got, ref, B, heads, Tn, grid, f"{variant} B={B} Tn={Tn} at the device's grid, run {rep}")
            assert msg is None, msg
