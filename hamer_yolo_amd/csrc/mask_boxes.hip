// hm_mask_boxes - the tight bounding box and the pixel count of a label in a label mask, for many (frame, label) queries in one
// call (include/hamer_hip.h, "Mask boxes"): the device form of `rows, cols = np.where(mask == label)` followed by four min / max.
//
// Everything is an integer; the box is finished with integer min / max / add atomics, so a query's five values depend on
// nothing but its own frame -- not on Q, the order of the queries, the rest of the batch or the grid.
//
// Two kernels on the stream, no host synchronisation, no allocation:
//   init   writes all five values of every query: -1, -1, -1, -1, 0.  The two minima are kept as UNSIGNED words, so -1
//          (0xffffffff) is the identity of atomicMin there and the "no such pixel" answer at once; the two maxima are signed and
//          start at -1 for the same reason.  No third kernel has to turn sentinels into the empty row.
//   scan   one workgroup of 256 threads per (query, 16 KiB of the query's frame).  The frame is walked as H * W consecutive
//          bytes, not row by row: from the first 16-byte aligned address on, every thread reads four 16-byte vectors (all four
//          loads are issued before any is looked at) and tests the 16 labels of each with word arithmetic; the up to 15 bytes
//          before the first aligned address and the up to 15 after the last whole vector are read one by one by the query's
//          first workgroup.  So W and H * W need not be multiples of anything and a row may start at any address.  A vector
//          without the label -- nearly all of them -- costs the four word tests.  One with the label turns its 16 answers into a
//          bit mask: when its bytes lie in one row the columns come from the mask's lowest and highest bit, otherwise (the
//          vector runs over a row's end, or W < 16) bit by bit.  Thread values are reduced in the wave with shuffles, the four
//          waves' through LDS, and thread 0 issues the five atomics when the workgroup saw the label at all.
//          A query whose frame is outside 0..N-1 is left as init wrote it; nothing of the mask is read for it.
//          Queries that share a frame each read it (the second read of 2 MB comes from the cache behind the first).
#include <stdint.h>
#include "common.h"
#include "hamer_hip_internal.h"

namespace {

constexpr int MB_THREADS = 256, MB_WAVES = MB_THREADS / 64, MB_UNROLL = 4;
constexpr long long MB_VECS = (long long)MB_THREADS * MB_UNROLL;           // 16-byte vectors per workgroup: 16 KiB

struct BoxParams {
  const uint8_t* mask; const hm_box_query* queries; int32_t* boxes;
  int N, H, W, Q;
  long long blocks_per_query;
};

struct Box { int x1, y1, x2, y2, n; };

__device__ __forceinline__ void box_add(Box& b, int x, int y) {
  b.x1 = x < b.x1 ? x : b.x1; b.x2 = x > b.x2 ? x : b.x2;
  b.y1 = y < b.y1 ? y : b.y1; b.y2 = y > b.y2 ? y : b.y2;
}

// 0x80 in every byte of w that belongs to the query: equal to the label, or non-zero for label -1 (exact: no carry crosses a byte)
__device__ __forceinline__ uint32_t match_bytes(uint32_t w, uint32_t pattern, bool any_label) {
  const uint32_t x = any_label ? w : w ^ pattern;
  const uint32_t zero = ~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x | 0x7f7f7f7fu);      // 0x80 where the byte of x is zero
  return any_label ? (~zero & 0x80808080u) : zero;
}

// the four 0x80 flags of a word -> bits 0..3 (byte 0, the lowest address, is bit 0)
__device__ __forceinline__ uint32_t pack4(uint32_t flags) { return (((flags >> 7) * 0x00204081u) >> 21) & 0xfu; }

__global__ __launch_bounds__(MB_THREADS) void mask_boxes_init_kernel(int32_t* boxes, long long n) {
  const long long i = (long long)blockIdx.x * MB_THREADS + threadIdx.x;
  if (i < n) boxes[i] = (i % 5 == 4) ? 0 : -1;
}

__global__ __launch_bounds__(MB_THREADS) void mask_boxes_scan_kernel(const BoxParams p) {
  __shared__ int red[MB_WAVES][5];
  const int q = (int)(blockIdx.x / p.blocks_per_query);
  const long long blk = blockIdx.x - (long long)q * p.blocks_per_query;
  const hm_box_query qu = p.queries[q];
  if (qu.frame < 0 || qu.frame >= p.N) return;                         // the whole workgroup leaves: nothing below is reached
  const bool any_label = qu.label == -1;
  const uint32_t pattern = (uint32_t)(qu.label & 0xff) * 0x01010101u;
  const bool possible = any_label || (qu.label >= 0 && qu.label <= 255);   // another label is in no byte: the row stays empty
  const int W = p.W;
  const int HW = p.H * p.W;                                             // < 2^31 (checked on the host)
  const uint8_t* __restrict__ fr = p.mask + (size_t)qu.frame * (size_t)HW;
  int head = (int)((16u - (unsigned)((uintptr_t)fr & 15u)) & 15u);      // bytes before the first 16-byte aligned address
  if (head > HW) head = HW;
  const int nvec = (HW - head) >> 4;
  const int tail0 = head + (nvec << 4);                                  // first byte behind the last whole vector
  Box b = {0x7fffffff, 0x7fffffff, -1, -1, 0};

  if (possible) {
    uint4 v[MB_UNROLL];
    int at[MB_UNROLL];
#pragma unroll
    for (int u = 0; u < MB_UNROLL; ++u) {
      const long long vi = blk * MB_VECS + (long long)u * MB_THREADS + threadIdx.x;
      at[u] = vi < nvec ? head + (int)(vi << 4) : -1;
      v[u] = make_uint4(0u, 0u, 0u, 0u);
      if (at[u] >= 0) v[u] = *reinterpret_cast<const uint4*>(fr + at[u]);          // at[u] + 15 < tail0 <= HW
    }
#pragma unroll
    for (int u = 0; u < MB_UNROLL; ++u) {
      if (at[u] < 0) continue;
      const uint32_t f0 = match_bytes(v[u].x, pattern, any_label), f1 = match_bytes(v[u].y, pattern, any_label);
      const uint32_t f2 = match_bytes(v[u].z, pattern, any_label), f3 = match_bytes(v[u].w, pattern, any_label);
      if ((f0 | f1 | f2 | f3) == 0u) continue;
      uint32_t m = pack4(f0) | (pack4(f1) << 4) | (pack4(f2) << 8) | (pack4(f3) << 12);
      const int y0 = at[u] / W, x0 = at[u] - y0 * W;
      b.n += __popc(m);
      if (x0 + 15 < W) {                                                // the 16 bytes lie in row y0
        box_add(b, x0 + (__ffs((int)m) - 1), y0);
        box_add(b, x0 + (31 - __clz((int)m)), y0);
      } else {
        while (m) {
          const int i = at[u] + (__ffs((int)m) - 1);
          m &= m - 1;
          const int y = i / W;
          box_add(b, i - y * W, y);
        }
      }
    }
    if (blk == 0) {
      // the scalar head (threads 0..15) and tail (threads 16..31) of the frame
      const int t = (int)threadIdx.x;
      int i = -1;
      if (t < head) i = t;
      else if (t >= 16 && t < 32 && tail0 + (t - 16) < HW) i = tail0 + (t - 16);
      if (i >= 0) {
        const int m = (int)fr[i];
        if (any_label ? m != 0 : m == qu.label) {
          const int y = i / W;
          box_add(b, i - y * W, y);
          b.n += 1;
        }
      }
    }
  }

  // wave, then workgroup, then the output
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) {
    const int ox1 = __shfl_xor(b.x1, s), oy1 = __shfl_xor(b.y1, s), ox2 = __shfl_xor(b.x2, s), oy2 = __shfl_xor(b.y2, s);
    b.x1 = ox1 < b.x1 ? ox1 : b.x1; b.y1 = oy1 < b.y1 ? oy1 : b.y1;
    b.x2 = ox2 > b.x2 ? ox2 : b.x2; b.y2 = oy2 > b.y2 ? oy2 : b.y2;
    b.n += __shfl_xor(b.n, s);
  }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { red[wave][0] = b.x1; red[wave][1] = b.y1; red[wave][2] = b.x2; red[wave][3] = b.y2; red[wave][4] = b.n; }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < MB_WAVES; ++w) {
      b.x1 = red[w][0] < b.x1 ? red[w][0] : b.x1; b.y1 = red[w][1] < b.y1 ? red[w][1] : b.y1;
      b.x2 = red[w][2] > b.x2 ? red[w][2] : b.x2; b.y2 = red[w][3] > b.y2 ? red[w][3] : b.y2;
      b.n += red[w][4];
    }
    if (b.n > 0) {
      int32_t* out = p.boxes + (size_t)q * 5;
      atomicMin(reinterpret_cast<unsigned int*>(out + 0), (unsigned int)b.x1);
      atomicMin(reinterpret_cast<unsigned int*>(out + 1), (unsigned int)b.y1);
      atomicMax(out + 2, b.x2);
      atomicMax(out + 3, b.y2);
      atomicAdd(out + 4, b.n);
    }
  }
}

}  // namespace

extern "C" int hm_mask_boxes(const uint8_t* mask, int N, int H, int W, const hm_box_query* queries, int Q, int32_t* boxes, void* stream_) {
  if (N < 1 || H < 1 || W < 1) return hm_set_error(HM_ERR_ARG, "hm_mask_boxes: N, H and W must be positive");
  if ((long long)N * H * W >= (1ll << 31)) return hm_set_error(HM_ERR_ARG, "hm_mask_boxes: N * H * W must be below 2^31");
  if (Q < 0) return hm_set_error(HM_ERR_ARG, "hm_mask_boxes: Q must not be negative");
  if (!mask) return hm_set_error(HM_ERR_ARG, "hm_mask_boxes: null mask");
  if (Q == 0) return HM_OK;                                              // nothing to box: no launch, nothing else is read
  if (!queries || !boxes) return hm_set_error(HM_ERR_ARG, "hm_mask_boxes: null queries or boxes");
  if (((uintptr_t)queries & 3) || ((uintptr_t)boxes & 3)) return hm_set_error(HM_ERR_ARG, "hm_mask_boxes: queries and boxes must be 4-byte aligned");
  BoxParams p;
  p.mask = mask; p.queries = queries; p.boxes = boxes; p.N = N; p.H = H; p.W = W; p.Q = Q;
  const long long vecs = ((long long)H * W) >> 4;                        // an upper bound of a frame's whole vectors
  p.blocks_per_query = vecs > 0 ? (vecs + MB_VECS - 1) / MB_VECS : 1;
  const long long blocks = p.blocks_per_query * Q, cells = (long long)Q * 5;
  if (blocks > 0x7fffffffll) return hm_set_error(HM_ERR_ARG, "hm_mask_boxes: Q * H * W too large for one call");
  hipStream_t s = (hipStream_t)stream_;
  HmProfScope prof(HM_K_OTHER, 3, Q, H, W, s);
  hipLaunchKernelGGL(mask_boxes_init_kernel, dim3((unsigned)((cells + MB_THREADS - 1) / MB_THREADS)), dim3(MB_THREADS), 0, s, boxes, cells);
  int rc = hm_check_launch("hm_mask_boxes (init)");
  if (rc != HM_OK) return rc;
  hipLaunchKernelGGL(mask_boxes_scan_kernel, dim3((unsigned)blocks), dim3(MB_THREADS), 0, s, p);
  return hm_check_launch("hm_mask_boxes (scan)");
}
