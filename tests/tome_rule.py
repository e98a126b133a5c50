"""Token merging stated plainly: bipartite_soft_matching and merge_wavg of the reference's ToMe backbone variant
(hamer/hamer/models/backbones/selective_vit_adapter.py:17-113), without class or distillation token, one crop at a time.

    tokens alternate between the sets A (even) and B (odd); every token is divided by its Euclidean norm
    score(a, j) = <A_a, B_j>
    A token a proposes best(a) = the LOWEST j among the maxima of score(a, .), with proposal score p(a) = that maximum
    the A tokens are ranked by p descending, the LOWER a first among equal p        (a stable descending sort)
    the first r of the ranking are merged away: src = those a, dst = best(a); the rest stay: unm, in ranking order
    out = [ A_unm ... | B_0 ... B_(Nb-1) ], B_j joined by every src whose dst is j:
        x_out = sum(x * size) / sum(size) over the group, size_out = sum(size)

Everything up to the final quotient is int64 / float64 torch arithmetic.  With ``exact=True`` (the data of
tests/exact_data.py: integer metric rows with integer norms, integer x and sizes) every intermediate is asserted to be exact
-- the squared norm a perfect square, every normalised value and every score unchanged by a round trip through fp32, the
weighted sums integers below 2^24 -- so the decisions do not depend on the order of any sum, and a kernel has to reproduce
them bit for bit.  The final quotient is one fp32 division of two exactly known fp32 numbers.  ``exact=False`` states the same
rule in float64 on any data (the fp32 kernels and the oracle then agree with it wherever no two scores are closer than
their rounding).

Plain helper module (imported like nms_rule.py); torch-CPU only, nothing here touches the compiled library or the oracle.
"""
import torch

EXACT_LIMIT = 1 << 24


def _f32_exact(t):
    return torch.equal(t.float().double(), t)


def scores(metric, exact=True):
    """metric (T, C) -> (Na, Nb) float64 cosines of the even tokens against the odd ones."""
    m = metric.double()
    ss = (m * m).sum(1)
    n = ss.sqrt()
    if exact:
        assert torch.equal(m, m.round()) and float(ss.max()) < EXACT_LIMIT
        n = n.round()
        assert torch.equal(n * n, ss) and float(n.min()) > 0, "the norms are not integers"
    m = m / n[:, None]
    s = m[0::2] @ m[1::2].t()
    if exact:
        assert _f32_exact(m) and _f32_exact(s) and _f32_exact(s * 4096) and torch.equal(s * 4096, (s * 4096).round())
    return s


def match_crop(metric, r, exact=True):
    """metric (T, C), 0 < r <= T // 2 -> (unm [Na - r], src [r], dst [r]) as lists of ints."""
    s = scores(metric, exact).tolist()
    best, prop = [], []
    for row in s:
        bj, bs = 0, row[0]
        for j, v in enumerate(row):
            if v > bs:                                   # a later equal score does not replace the first maximum
                bj, bs = j, v
        best.append(bj)
        prop.append(bs)
    order = sorted(range(len(s)), key=lambda a: (-prop[a], a))
    return order[r:], order[:r], [best[a] for a in order[:r]]


def match(metric, r, exact=True):
    """metric (B, T, C) -> int64 (unm (B, Na - r), src (B, r), dst (B, r))."""
    per = [match_crop(m, r, exact) for m in metric]
    B = len(per)
    return tuple(torch.tensor([p[k] for p in per], dtype=torch.int64).reshape(B, -1) for k in range(3))


def group_sums(x, size, unm, src, dst, exact=True):
    """float64 (sum of x * size (B, T - r, D), sum of size (B, T - r)) over every group of the output."""
    B, T, D = x.shape
    size = torch.ones(B, T, dtype=x.dtype) if size is None else size
    nums, dens = [], []
    for b in range(B):
        xw = x[b].double() * size[b].double()[:, None]
        sz = size[b].double()
        num = [xw[2 * a] for a in unm[b].tolist()] + [xw[2 * j + 1].clone() for j in range(T // 2)]
        den = [sz[2 * a] for a in unm[b].tolist()] + [sz[2 * j + 1].clone() for j in range(T // 2)]
        first_b = unm.shape[1]
        for a, j in zip(src[b].tolist(), dst[b].tolist()):
            num[first_b + j] += xw[2 * a]
            den[first_b + j] += sz[2 * a]
        num, den = torch.stack(num), torch.stack(den)
        if exact:
            assert torch.equal(num, num.round()) and torch.equal(den, den.round())
            assert float(num.abs().max()) < EXACT_LIMIT and float(den.max()) < EXACT_LIMIT
        nums.append(num)
        dens.append(den)
    return torch.stack(nums), torch.stack(dens)


def merge(x, size, unm, src, dst, exact=True):
    """x (B, T, D), size (B, T) or None (all ones), the matching -> fp32 (x_out (B, T - r, D), size_out (B, T - r))."""
    num, den = group_sums(x, size, unm, src, dst, exact)
    return num.float() / den.float()[..., None], den.float()          # the one rounding: an fp32 division of exact operands


def quotient_representable(x, size, unm, src, dst):
    """bool (B, T - r, D): where the exact quotient is an fp32 number, so that even a division that is not correctly rounded
    in the last place has one right answer (every unmerged row is such a place)."""
    num, den = group_sums(x, size, unm, src, dst)
    q = num.float() / den.float()[..., None]
    return q.double() * den[..., None] == num
