"""GPU: hm_mask_boxes (csrc/mask_boxes.hip) against the numpy rule of tests/mask_boxes_rule.py -- integers, so equality --
on the smallest shapes that can break it: odd widths, frames and rows that start at no multiple of 16 bytes, a frame smaller
than one load, labels only in the first / last pixel or only in the bytes the kernel reads one by one, empty and full frames,
frames outside the batch, queries that share a frame, every query alone against itself inside the batch, an output buffer full
of garbage, Q == 0 and every refused argument."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mask_boxes_rule as BR  # noqa: E402

from hamer_yolo_amd import lib as L  # noqa: E402
from hamer_yolo_amd.hamer.utils import mask_eval as ME  # noqa: E402

SHAPES = [(2, 37, 53), (3, 5, 131), (1, 1, 1), (1, 64, 4096)]
GARBAGE = -0x5a5a5a5b


def _upload(mask: np.ndarray, offset: int = 0) -> torch.Tensor:
    """The mask on the device, ``offset`` bytes past an allocation's start (so that the first frame is not 16-byte aligned)."""
    flat = torch.zeros(mask.size + offset + 16, dtype=torch.uint8, device="cuda")
    view = flat[offset:offset + mask.size].view(mask.shape)
    view.copy_(torch.from_numpy(mask))
    assert view.is_contiguous() and flat.data_ptr() % 16 == 0 and view.data_ptr() % 16 == offset % 16
    return view


def _run(dev_mask, queries) -> np.ndarray:
    out = torch.full((len(queries), 5), GARBAGE, dtype=torch.int32, device="cuda")     # callers do not clear the buffer
    got = ME.mask_boxes(dev_mask, queries, boxes=out)
    assert got is out
    return out.cpu().numpy()


def _check(mask: np.ndarray, queries, offset: int = 0) -> np.ndarray:
    dev = _upload(mask, offset)
    want = BR.boxes(mask, queries)
    got = _run(dev, queries)
    np.testing.assert_array_equal(got, want)
    for q, query in enumerate(queries):                       # each query alone: the same integers as inside the batch
        np.testing.assert_array_equal(_run(dev, [query])[0], got[q], err_msg=str(query))
    np.testing.assert_array_equal(_run(dev, list(reversed(queries))), want[::-1])
    return got


def _sparse(N, H, W, seed):
    rng = np.random.default_rng(seed)
    m = np.zeros((N, H, W), np.uint8)
    for n in range(N):
        for label in (1, 3, 4, 255):
            k = max(1, (H * W) // 97)
            m[n, rng.integers(0, H, k), rng.integers(0, W, k)] = label
    return m


@pytest.mark.parametrize("offset", [0, 3])
@pytest.mark.parametrize("shape", SHAPES)
def test_kernel_equals_the_rule(shape, offset):
    N, H, W = shape
    m = _sparse(N, H, W, 11 * H + W)
    queries = [(n, label) for n in range(N) for label in (3, 4, 7, -1, 0)]
    queries += [(-1, 3), (N, 3), (0, 255), (0, 256), (0, -2)]                 # frames outside the batch; labels in no byte
    got = _check(m, queries, offset)
    assert got[-5].tolist() == got[-4].tolist() == got[-2].tolist() == got[-1].tolist() == list(BR.EMPTY)
    assert N * H * W == 1 or (got[:, 4] > 0).any()


@pytest.mark.parametrize("offset", [0, 3, 15])
def test_single_pixels_corners_and_the_bytes_read_one_by_one(offset):
    N, H, W = 2, 37, 53                                        # H W = 1961: frame 1 starts 9 bytes past frame 0's alignment
    HW = H * W
    cases = [[(0, 0)], [(H - 1, W - 1)], [(0, 0), (H - 1, W - 1)], [(17, 29)],
             [(y, 0) for y in range(H)], [(y, W - 1) for y in range(H)], [(5, x) for x in range(W)]]
    for n in range(N):
        # the bytes before the frame's first 16-byte aligned address and behind its last whole vector, alone and together
        head = (-(offset + n * HW)) % 16
        tail = (HW - head) % 16
        flat_cases = [list(range(head)), list(range(HW - tail, HW)), [head - 1] if head else [0], [HW - tail] if tail else [HW - 1],
                      [max(head - 1, 0), head], [HW - tail - 1, min(HW - tail, HW - 1)]]
        for pix in cases + [[divmod(i, W) for i in flat] for flat in flat_cases if flat]:
            m = np.zeros((N, H, W), np.uint8)
            m[1 - n] = 3                                        # the other frame is full of the label: it must not leak in
            for y, x in pix:
                m[n, y, x] = 3
            got = _check(m, [(n, 3), (n, -1), (1 - n, 3)], offset)
            assert got[0, 4] == len(set(pix)) and got[2].tolist() == [0, 0, W - 1, H - 1, HW]


def test_rows_shorter_than_a_vector_and_vectors_across_row_ends():
    for N, H, W in ((2, 40, 1), (1, 33, 7), (3, 9, 15), (1, 3, 17), (2, 2, 16)):
        m = _sparse(N, H, W, 5 * W + H)
        m[:, H - 1, W - 1] = 4
        _check(m, [(n, label) for n in range(N) for label in (3, 4, -1)], offset=5)
        full = np.full((N, H, W), 3, np.uint8)
        assert _check(full, [(N - 1, 3), (0, 4)])[:, 4].tolist() == [H * W, 0]


def test_one_full_hd_frame():
    H, W = 1080, 1920
    m = np.zeros((1, H, W), np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    m[0][(yy - 500) ** 2 + (xx - 1211) ** 2 < 150 ** 2] = 3                    # a blob the size of a hand
    m[0][(yy - 200) ** 2 + (xx - 300) ** 2 < 90 ** 2] = 4
    m[0, 1079, 1919] = 9
    dev = _upload(m)
    queries = [(0, 3), (0, 4), (0, 9), (0, 5), (0, -1)]
    got = _run(dev, queries)
    np.testing.assert_array_equal(got, BR.boxes(m, queries))
    assert got[0].tolist()[:4] == [1211 - 149, 500 - 149, 1211 + 149, 500 + 149] and got[2].tolist() == [1919, 1079, 1919, 1079, 1]
    for q, query in enumerate(queries):
        np.testing.assert_array_equal(_run(dev, [query])[0], got[q])
    full = torch.full((1, H, W), 3, dtype=torch.uint8, device="cuda")
    assert _run(full, [(0, 3), (0, -1), (0, 4)]).tolist() == [[0, 0, W - 1, H - 1, H * W]] * 2 + [list(BR.EMPTY)]


def test_queries_that_share_a_frame_next_to_one_that_does_not():
    m = _sparse(3, 45, 77, 3)
    queries = [(1, 3), (1, 4), (1, -1), (1, 3), (2, 1)]
    got = _check(m, queries, offset=7)
    assert got[0].tolist() == got[3].tolist() and got[0, 4] > 0 and got[4, 4] > 0
    many = [(n % 3, (3, 4, 1, 255, -1)[n % 5]) for n in range(300)]                # more queries than a workgroup has threads
    np.testing.assert_array_equal(_run(_upload(m), many), BR.boxes(m, many))


def test_no_query_and_tensor_queries():
    m = _upload(_sparse(2, 20, 30, 1))
    assert tuple(ME.mask_boxes(m, []).shape) == (0, 5)
    lib = L.load()
    out = torch.full((4, 5), GARBAGE, dtype=torch.int32, device="cuda")
    qd = torch.tensor([[0, 3], [1, 4], [5, 3], [1, -1]], dtype=torch.int32, device="cuda")
    assert lib.hm_mask_boxes(L.ptr(m), 2, 20, 30, L.ptr(qd), 0, L.ptr(out), L.current_stream()) == 0
    torch.cuda.synchronize()
    assert (out == GARBAGE).all()                                                  # Q == 0 launched nothing
    ME.mask_boxes(m, qd, boxes=out)                                                # queries already on the device
    np.testing.assert_array_equal(out.cpu().numpy(), BR.boxes(m.cpu().numpy(), [(0, 3), (1, 4), (5, 3), (1, -1)]))
    for bad in (m[:, :, :7], m.to(torch.int32), m[0]):
        with pytest.raises(ValueError):
            ME.mask_boxes(bad, [(0, 3)])
    with pytest.raises(ValueError):
        ME.mask_boxes(m, [(0, 3)], boxes=torch.empty(2, 5, dtype=torch.int32, device="cuda"))


def test_refused_arguments_touch_nothing():
    m = _upload(_sparse(2, 20, 30, 2))
    lib = L.load()
    out = torch.full((3, 5), GARBAGE, dtype=torch.int32, device="cuda")
    qd = torch.tensor([[0, 3], [1, 4], [0, -1]], dtype=torch.int32, device="cuda")
    good = dict(mask=L.ptr(m), N=2, H=20, W=30, queries=L.ptr(qd), Q=3, boxes=L.ptr(out))
    for kw in (dict(mask=None), dict(queries=None), dict(boxes=None), dict(N=0), dict(H=0), dict(W=0), dict(N=-2), dict(Q=-1),
               dict(N=1 << 11, H=1 << 10, W=1 << 10), dict(queries=L.ptr(qd) + 2), dict(boxes=L.ptr(out) + 1)):
        a = dict(good, **kw)
        rc = lib.hm_mask_boxes(a["mask"], a["N"], a["H"], a["W"], a["queries"], a["Q"], a["boxes"], L.current_stream())
        assert rc == -1 and "hm_mask_boxes" in lib.hm_last_error_string().decode(), kw     # HM_ERR_ARG
    torch.cuda.synchronize()
    assert (out == GARBAGE).all()
    assert lib.hm_mask_boxes(*[good[k] for k in ("mask", "N", "H", "W", "queries", "Q", "boxes")], L.current_stream()) == 0
    np.testing.assert_array_equal(out.cpu().numpy(), BR.boxes(m.cpu().numpy(), [(0, 3), (1, 4), (0, -1)]))
