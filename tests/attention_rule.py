"""Plain statement of the attention kernels (csrc/attention.hip, csrc/attention_f32.hip, hm_tome_attention) in float64, for the
exact-data tests: softmax(c q k^T + log2(size)) v in the log2 domain, with the one property of an fp32 exponential the exact
data rests on stated explicitly -- a probability below the smallest fp32 subnormal, 2^-149 of the row maximum, is zero.

`fault` names one index mistake of the MFMA kernel's maps (tests/test_exact_data_host.py applies each to the rule and requires
the exact data to see it).  Torch on the CPU only; nothing here touches the compiled library.
"""
import torch

FAULTS = ["V read without the slot permutation", "V rows of neighbouring 16-key tiles swapped", "V rows of the previous item",
          "head index off by one", "query rows of neighbouring tiles swapped", "columns dt*16 + 4g permuted across g",
          "one key tile dropped"]
DROPPED_TILE = 5


def _ar(n):
    return torch.arange(n, dtype=torch.int64)


def v_key_map(fault, T):
    """Key whose V row the product takes for the P of key t (identity without a fault; a map never leaves 0..T-1)."""
    t = _ar(T)
    if fault == "V read without the slot permutation":
        # slot (g, j) of a 32-key step holds P of key 4g + j (j < 4) and 16 + 4g + (j - 4) (j >= 4); V read as key 4g + j
        kk, r = t // 32, t % 32
        g, j = (r % 16) // 4, r % 4
        bad = kk * 32 + 4 * g + 4 + j
        m = torch.where(r >= 16, bad, t)
    elif fault == "V rows of neighbouring 16-key tiles swapped":
        m = (t // 16 ^ 1) * 16 + t % 16
    else:
        return t
    return torch.where(m < T, m, t)


def attention_rule(q, k, v, c, log2size=None, fault=None):
    """q, k, v (B, heads, T, d) float64, c the log2-domain scale, log2size (B, T) or None -> (B, heads, T, d) float64."""
    B, H, T, d = q.shape
    assert fault is None or fault in FAULTS
    if fault == "query rows of neighbouring tiles swapped" and T >= 32:
        qm = (_ar(T) // 16 ^ 1) * 16 + _ar(T) % 16
        q = q[:, :, torch.where(qm < T, qm, _ar(T))]
    z = (q @ k.transpose(-1, -2)) * c
    if log2size is not None:
        z = z + log2size[:, None, None, :]
    if fault == "one key tile dropped":
        tile = min(DROPPED_TILE, (T - 1) // 16)
        z = z.clone()
        z[..., tile * 16:tile * 16 + 16] = -float("inf")
    zmax = z.amax(-1, keepdim=True)
    p = torch.exp2(z - torch.where(zmax.isfinite(), zmax, torch.zeros_like(zmax)))
    p = torch.where(p < 2.0 ** -149, torch.zeros_like(p), p)
    vv = v[:, :, v_key_map(fault, T)]
    if fault == "V rows of the previous item":
        vv = vv.reshape(B * H, T, d).roll(1, 0).reshape(B, H, T, d)
    out = (p @ vv) / p.sum(-1, keepdim=True)
    if fault == "head index off by one":
        out = out.roll(-1, 1)
    if fault == "columns dt*16 + 4g permuted across g":
        col = _ar(d)
        out = out[..., (col // 16) * 16 + 4 * ((col % 16 // 4 + 1) % 4) + col % 4]
    return out
