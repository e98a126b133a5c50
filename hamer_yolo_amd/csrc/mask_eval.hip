// hm_mask_score - region similarity J and contour accuracy F of predicted silhouettes against label masks: the eight integer
// counts of include/hamer_hip.h ("Mask scores") per query, from which J, precision, recall and F are single divisions.
//
// Everything here is integer and bit arithmetic; the sums are integer atomics, so a query's counts depend on nothing but its
// own two images and the radius -- not on Q, the order of the queries, the rest of the batch or the grid.
//
// Three kernels on the stream, no host synchronisation, no allocation:
//   init   writes all 8 counts of every query: zeros and pixels = H * W (0 when the query's frame is outside 0..N-1; the other
//          two kernels then skip the query, so nothing is read out of bounds).
//   pack   the boundary pack of mask_bits.h, shared with mask_fit.hip, writes the two boundary maps to the workspace; on the way
//          areas, intersection and boundary counts are popcounts, added with one 64-bit atomic per wave and count when not zero.
//   match  one wave per (query, side, 64 consecutive words of that side's boundary map).  Lane i reads word i; the words that
//          hold a boundary pixel are then taken one at a time by the whole wave, lane j owning the row offsets dy = j - r,
//          j + 64 - r and j + 128 - r (2 r + 1 <= 129 of them): it
//          reads the three words of the OTHER map around (y + dy, c), dilates them along x by w(dy) = floor(sqrt(r r - dy dy))
//          with shift-and-OR doubling (the table of w comes from the host in integer arithmetic), and the OR over the lanes is
//          the other boundary dilated by the disk, restricted to this word.  matched += popcount(word & that).  Most words hold
//          no boundary pixel and cost one load.
#include "common.h"
#include "mask_bits.h"

namespace {
using namespace mask_bits;

struct MaskParams : Params {
  unsigned long long* counts;                            // [Q][8]
};

__global__ __launch_bounds__(THREADS) void mask_init_kernel(const MaskParams p) {
  const long long i = (long long)blockIdx.x * THREADS + threadIdx.x;
  if (i >= (long long)p.Q * 8) return;
  const int q = (int)(i >> 3), k = (int)(i & 7);
  const int frame = p.queries[q].frame;
  const bool ok = frame >= 0 && frame < p.N;
  p.counts[i] = (k == 7 && ok) ? (unsigned long long)p.H * (unsigned long long)p.W : 0ull;
}

__global__ __launch_bounds__(THREADS) void mask_pack_kernel(const MaskParams p) {
  unsigned long long inter = 0, pa = 0, ga = 0, pb = 0, gb = 0;
  const int q = pack_strips(p, [&](const RowWords& cur, unsigned long long bpw, unsigned long long bgw, unsigned long long valid) {
    inter += __popcll(cur.p & cur.g & valid); pa += __popcll(cur.p & valid); ga += __popcll(cur.g & valid);
    pb += __popcll(bpw); gb += __popcll(bgw);
  });
  if (q >= 0 && (threadIdx.x & 63) == 0) {
    unsigned long long* cnt = p.counts + (size_t)q * 8;
    if (inter) atomicAdd(cnt + 0, inter);
    if (pa) atomicAdd(cnt + 1, pa);
    if (ga) atomicAdd(cnt + 2, ga);
    if (pb) atomicAdd(cnt + 3, pb);
    if (gb) atomicAdd(cnt + 4, gb);
  }
}

// (hi:lo) |= (hi:lo) << s, 1 <= s <= 63
__device__ __forceinline__ void or_shl(unsigned long long& hi, unsigned long long& lo, int s) {
  hi |= (hi << s) | (lo >> (64 - s));
  lo |= lo << s;
}
__device__ __forceinline__ void or_shr(unsigned long long& hi, unsigned long long& lo, int s) {
  lo |= (lo >> s) | (hi << (64 - s));
  hi |= hi >> s;
}

// The middle word of the row (below : mid : above, ascending x) dilated along x by w pixels, 0 <= w <= 64: OR of the shifts
// 0..w both ways.  Doubling: after the loop acc holds the shifts 0..span-1 with span <= w + 1 < 2 span; one more shift by
// w + 1 - span (< span) closes the range.  No shift exceeds 32.
__device__ __forceinline__ unsigned long long dilate_word(unsigned long long below, unsigned long long mid, unsigned long long above, int w) {
  unsigned long long uh = mid, ul = below, dh = above, dl = mid;       // up: towards larger x, read from uh; down: from dl
  int span = 1;
  while (2 * span <= w + 1) { or_shl(uh, ul, span); or_shr(dh, dl, span); span *= 2; }
  const int rest = w + 1 - span;
  if (rest > 0) { or_shl(uh, ul, rest); or_shr(dh, dl, rest); }
  return uh | dl;
}

__global__ __launch_bounds__(THREADS) void mask_match_kernel(const MaskParams p) {
  const int lane = threadIdx.x & 63;
  const long long items = (long long)p.H * p.words;
  const long long chunks = (items + 63) / 64;
  const long long task = (long long)blockIdx.x * WAVES + (threadIdx.x >> 6);
  if (task >= chunks * 2 * p.Q) return;
  const int q = (int)(task / (chunks * 2));
  const long long rem = task - (long long)q * chunks * 2;
  const int side = (int)(rem / chunks);
  const long long chunk = rem - (long long)side * chunks;
  const int frame = p.queries[q].frame;
  if (frame < 0 || frame >= p.N) return;
  const unsigned long long* __restrict__ mine = p.bits + ((size_t)q * 2 + side) * (size_t)items;
  const unsigned long long* __restrict__ other = p.bits + ((size_t)q * 2 + (1 - side)) * (size_t)items;
  const long long item = chunk * 64 + lane;
  const unsigned long long word = item < items ? mine[item] : 0ull;
  unsigned long long active = __ballot(word != 0ull);
  unsigned long long matched = 0;
  if (!active) return;
  int wj[3];                                                            // this lane's half widths: dy = lane + 64 k - r, k = 0..2
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int dy = lane + 64 * k - p.r, ad = dy < 0 ? -dy : dy;
    wj[k] = ad <= p.r ? (int)p.hw[ad] : -1;                             // -1: past the disk (2 r + 1 <= 129 offsets in all)
  }
  while (active) {
    const int src = __ffsll((long long)active) - 1;
    active &= active - 1;
    const unsigned a_lo = __shfl((unsigned)word, src), a_hi = __shfl((unsigned)(word >> 32), src);
    const unsigned long long a = ((unsigned long long)a_hi << 32) | a_lo;
    const long long it = chunk * 64 + src;
    const int y = (int)(it / p.words), c = (int)(it - (long long)y * p.words);
    unsigned long long d = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int yy = y + lane + 64 * k - p.r;
      if (wj[k] < 0 || yy < 0 || yy >= p.H) continue;
      const unsigned long long* __restrict__ row = other + (size_t)yy * p.words;
      const unsigned long long below = c > 0 ? row[c - 1] : 0ull, mid = row[c], above = c + 1 < p.words ? row[c + 1] : 0ull;
      if ((below | mid | above) == 0ull) continue;
      d |= dilate_word(below, mid, above, wj[k]);
    }
    d &= a;                                                             // only this word's boundary pixels matter
    unsigned d_lo = (unsigned)d, d_hi = (unsigned)(d >> 32);
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) { d_lo |= __shfl_xor(d_lo, s); d_hi |= __shfl_xor(d_hi, s); }
    matched += __popc(d_lo) + __popc(d_hi);
  }
  if (lane == 0 && matched) atomicAdd(p.counts + (size_t)q * 8 + 5 + side, matched);
}

}  // namespace

extern "C" size_t hm_mask_score_workspace_bytes(int Q, int H, int W, int radius) {
  if (Q < 0 || H < 1 || W < 1 || radius < 0 || radius > MAX_RADIUS) return 0;
  return map_words(Q < 1 ? 1 : Q, H, W) * sizeof(unsigned long long);    // never 0 for legal sizes: Q == 0 asks for one query's
}

extern "C" int hm_mask_score(const int32_t* pred_id, const uint8_t* mask, int N, int H, int W, const hm_mask_query* queries, int Q,
                             int radius, int64_t* counts, void* workspace, size_t workspace_bytes, void* stream_) {
  MaskParams p;
  p.pred = pred_id; p.mask = mask; p.queries = queries;
  p.N = N; p.H = H; p.W = W; p.Q = Q; p.r = radius;
  p.counts = (unsigned long long*)counts; p.bits = (unsigned long long*)workspace;
  const char* buffers = (!queries || !counts || !workspace) ? "null queries, counts or workspace"
      : workspace_bytes < hm_mask_score_workspace_bytes(Q, H, W, radius) ? "workspace too small (hm_mask_score_workspace_bytes)"
      : (((uintptr_t)counts & 7) || ((uintptr_t)workspace & 7) || ((uintptr_t)pred_id & 3) || ((uintptr_t)queries & 3))
          ? "counts and workspace must be 8-byte aligned, pred_id and queries 4-byte" : nullptr;
  int rc = host_checks("hm_mask_score", p, nullptr, buffers);
  if (rc != HM_OK || Q == 0) return rc;                                  // no query, nothing to score: no launch
  const long long chunks = ((long long)H * p.words + 63) / 64;
  const long long match_blocks = ((long long)Q * 2 * chunks + WAVES - 1) / WAVES;
  if (pack_blocks(p) > 0x7fffffffll || match_blocks > 0x7fffffffll)
    return hm_set_error(HM_ERR_ARG, "hm_mask_score: Q * H * W too large for one call");
  hipStream_t s = (hipStream_t)stream_;
  HmProfScope prof(HM_K_OTHER, 2, Q, H, W, s);
  hipLaunchKernelGGL(mask_init_kernel, dim3((unsigned)(((long long)Q * 8 + THREADS - 1) / THREADS)), dim3(THREADS), 0, s, p);
  rc = hm_check_launch("hm_mask_score (init)");
  if (rc != HM_OK) return rc;
  hipLaunchKernelGGL(mask_pack_kernel, dim3((unsigned)pack_blocks(p)), dim3(THREADS), 0, s, p);
  rc = hm_check_launch("hm_mask_score (pack)");
  if (rc != HM_OK) return rc;
  hipLaunchKernelGGL(mask_match_kernel, dim3((unsigned)match_blocks), dim3(THREADS), 0, s, p);
  return hm_check_launch("hm_mask_score (match)");
}
