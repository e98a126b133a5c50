// hm_mask_score - region similarity J and contour accuracy F of predicted silhouettes against label masks: the eight integer
// counts of include/hamer_hip.h ("Mask scores") per query, from which J, precision, recall and F are single divisions.
//
// Everything here is integer and bit arithmetic; the sums are integer atomics, so a query's counts depend on nothing but its
// own two images and the radius -- not on Q, the order of the queries, the rest of the batch or the grid.
//
// Three kernels on the stream, no host synchronisation, no allocation:
//   init   writes all 8 counts of every query: zeros and pixels = H * W (0 when the query's frame is outside 0..N-1; the other
//          two kernels then skip the query, so nothing is read out of bounds).
//   pack   one wave per (query, strip of 32 rows, 64-pixel word of a row).  Lane l reads pixel x = 64 c + l (clamped to W - 1:
//          the replicated last column) of one row; __ballot turns the wave's 64 answers into one word of the pred image and one
//          of the gt image.  Lane 63 also reads pixel 64 c + 64 (clamped), the east neighbour of the word's last pixel.  With
//          the word of the next row (clamped to H - 1: the replicated last row) the boundary map is three XORs of whole words:
//            b = ((s ^ east(s)) | (s ^ south) | (s ^ east(south))) & valid,   east(w) = (w >> 1) | (extra << 63).
//          The two boundary words go to the workspace ([Q][2][H][ceil(W / 64)] uint64, bits at or past W are zero); areas,
//          intersection and boundary counts are popcounts, added with one 64-bit atomic per wave and count when not zero.
//          The south rows of 8 rows are loaded before any is used, so a wave has 16 row loads in flight.
//   match  one wave per (query, side, 64 consecutive words of that side's boundary map).  Lane i reads word i; the words that
//          hold a boundary pixel are then taken one at a time by the whole wave, lane j owning the row offsets dy = j - r,
//          j + 64 - r and j + 128 - r (2 r + 1 <= 129 of them): it
//          reads the three words of the OTHER map around (y + dy, c), dilates them along x by w(dy) = floor(sqrt(r r - dy dy))
//          with shift-and-OR doubling (the table of w comes from the host in integer arithmetic), and the OR over the lanes is
//          the other boundary dilated by the disk, restricted to this word.  matched += popcount(word & that).  Most words hold
//          no boundary pixel and cost one load.
#include <stdint.h>
#include <stdio.h>
#include "common.h"
#include "hamer_hip_internal.h"

namespace {

constexpr int MK_MAX_RADIUS = 64, MK_STRIP = 32, MK_GROUP = 8, MK_THREADS = 256, MK_WAVES = MK_THREADS / 64;

struct MaskParams {
  const int32_t* pred; const uint8_t* mask; const hm_mask_query* queries;
  int N, H, W, Q, r, words;                              // words = ceil(W / 64)
  unsigned long long* counts;                            // [Q][8]
  unsigned long long* bits;                              // [Q][2][H][words]
  uint8_t hw[MK_MAX_RADIUS + 1];                         // hw[d] = floor(sqrt(r r - d d)) for d <= r
};

__global__ __launch_bounds__(MK_THREADS) void mask_init_kernel(const MaskParams p) {
  const long long i = (long long)blockIdx.x * MK_THREADS + threadIdx.x;
  if (i >= (long long)p.Q * 8) return;
  const int q = (int)(i >> 3), k = (int)(i & 7);
  const int frame = p.queries[q].frame;
  const bool ok = frame >= 0 && frame < p.N;
  p.counts[i] = (k == 7 && ok) ? (unsigned long long)p.H * (unsigned long long)p.W : 0ull;
}

// one row's words: the pred and gt answers of the wave's 64 pixels, and of the pixel east of the last one (bit 63 of e*)
struct RowWords { unsigned long long p, g, ep, eg; };
// what a lane reads of one row: its own pixel and, in lane 63 alone, the pixel east of the word
struct RowPixels { int id, m, ide, me; };

__device__ __forceinline__ RowPixels load_row(const int32_t* __restrict__ pr, const uint8_t* __restrict__ mk, int xc, int xe, bool last_lane) {
  RowPixels v;
  v.id = pr[xc]; v.m = (int)mk[xc]; v.ide = -1; v.me = 0;
  if (last_lane) { v.ide = pr[xe]; v.me = (int)mk[xe]; }
  return v;
}

__device__ __forceinline__ RowWords row_words(const RowPixels v, bool last_lane, int lo, int hi, int label) {
  const bool ps = v.id >= lo && v.id < hi, gs = label == -1 ? v.m != 0 : v.m == label;
  const bool pe = last_lane && v.ide >= lo && v.ide < hi, ge = last_lane && (label == -1 ? v.me != 0 : v.me == label);
  RowWords w;
  w.p = __ballot(ps); w.g = __ballot(gs);
  w.ep = __ballot(pe) ? 1ull << 63 : 0ull;
  w.eg = __ballot(ge) ? 1ull << 63 : 0ull;
  return w;
}

__global__ __launch_bounds__(MK_THREADS) void mask_pack_kernel(const MaskParams p) {
  const int lane = threadIdx.x & 63;
  const bool last_lane = lane == 63;
  const int strips = (p.H + MK_STRIP - 1) / MK_STRIP;
  const long long per_query = (long long)strips * p.words;
  const long long task = (long long)blockIdx.x * MK_WAVES + (threadIdx.x >> 6);
  if (task >= per_query * p.Q) return;                                  // a whole wave leaves: nothing below synchronises
  const int q = (int)(task / per_query);
  const int rem = (int)(task - (long long)q * per_query);
  const int strip = rem / p.words, c = rem - strip * p.words;
  const hm_mask_query qu = p.queries[q];
  if (qu.frame < 0 || qu.frame >= p.N) return;
  const int x = c * 64 + lane;
  const int xc = x < p.W ? x : p.W - 1, xe = c * 64 + 64 < p.W ? c * 64 + 64 : p.W - 1;
  const unsigned long long valid = __ballot(x < p.W);
  const size_t plane = (size_t)p.H * (size_t)p.W;
  const int32_t* __restrict__ pr = p.pred + (size_t)qu.frame * plane;
  const uint8_t* __restrict__ mk = p.mask + (size_t)qu.frame * plane;
  unsigned long long* __restrict__ bp = p.bits + ((size_t)q * 2 + 0) * (size_t)p.H * p.words;
  unsigned long long* __restrict__ bg = p.bits + ((size_t)q * 2 + 1) * (size_t)p.H * p.words;
  const int y0 = strip * MK_STRIP, y_end = y0 + MK_STRIP < p.H ? y0 + MK_STRIP : p.H;
  unsigned long long inter = 0, pa = 0, ga = 0, pb = 0, gb = 0;
  RowWords cur = row_words(load_row(pr + (size_t)y0 * p.W, mk + (size_t)y0 * p.W, xc, xe, last_lane), last_lane, qu.id_lo, qu.id_hi, qu.label);
  for (int yb = y0; yb < y_end; yb += MK_GROUP) {
    // the south rows of MK_GROUP rows are read before any is used: the loads of a group are in flight together.  A row index is
    // clamped to H - 1, so the last row's south neighbour is itself and no load leaves the image
    RowPixels south[MK_GROUP];
#pragma unroll
    for (int k = 0; k < MK_GROUP; ++k) {
      const int ys = yb + 1 + k < p.H ? yb + 1 + k : p.H - 1;
      south[k] = load_row(pr + (size_t)ys * p.W, mk + (size_t)ys * p.W, xc, xe, last_lane);
    }
#pragma unroll
    for (int k = 0; k < MK_GROUP; ++k) {
      const int y = yb + k;
      if (y >= y_end) break;
      const RowWords nxt = row_words(south[k], last_lane, qu.id_lo, qu.id_hi, qu.label);
      const unsigned long long pe = (cur.p >> 1) | cur.ep, pse = (nxt.p >> 1) | nxt.ep;
      const unsigned long long ge = (cur.g >> 1) | cur.eg, gse = (nxt.g >> 1) | nxt.eg;
      const unsigned long long bpw = ((cur.p ^ pe) | (cur.p ^ nxt.p) | (cur.p ^ pse)) & valid;
      const unsigned long long bgw = ((cur.g ^ ge) | (cur.g ^ nxt.g) | (cur.g ^ gse)) & valid;
      if (lane == 0) {
        bp[(size_t)y * p.words + c] = bpw;
        bg[(size_t)y * p.words + c] = bgw;
      }
      inter += __popcll(cur.p & cur.g & valid); pa += __popcll(cur.p & valid); ga += __popcll(cur.g & valid);
      pb += __popcll(bpw); gb += __popcll(bgw);
      cur = nxt;
    }
  }
  if (lane == 0) {
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

__global__ __launch_bounds__(MK_THREADS) void mask_match_kernel(const MaskParams p) {
  const int lane = threadIdx.x & 63;
  const long long items = (long long)p.H * p.words;
  const long long chunks = (items + 63) / 64;
  const long long task = (long long)blockIdx.x * MK_WAVES + (threadIdx.x >> 6);
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

long long mask_words(int W) { return ((long long)W + 63) / 64; }

}  // namespace

extern "C" size_t hm_mask_score_workspace_bytes(int Q, int H, int W, int radius) {
  if (Q < 0 || H < 1 || W < 1 || radius < 0 || radius > MK_MAX_RADIUS) return 0;
  const size_t per_query = (size_t)2 * (size_t)H * (size_t)mask_words(W) * sizeof(unsigned long long);
  return (size_t)(Q < 1 ? 1 : Q) * per_query;                            // never 0 for legal sizes: Q == 0 asks for one query's
}

extern "C" int hm_mask_score(const int32_t* pred_id, const uint8_t* mask, int N, int H, int W, const hm_mask_query* queries, int Q,
                             int radius, int64_t* counts, void* workspace, size_t workspace_bytes, void* stream_) {
  if (N < 1 || H < 1 || W < 1) return hm_set_error(HM_ERR_ARG, "hm_mask_score: N, H and W must be positive");
  if ((long long)N * H * W >= (1ll << 31)) return hm_set_error(HM_ERR_ARG, "hm_mask_score: N * H * W must be below 2^31");
  if (radius < 0 || radius > MK_MAX_RADIUS) return hm_set_error(HM_ERR_ARG, "hm_mask_score: radius must be in 0..64");
  if (Q < 0) return hm_set_error(HM_ERR_ARG, "hm_mask_score: Q must not be negative");
  if (!pred_id || !mask) return hm_set_error(HM_ERR_ARG, "hm_mask_score: null pred_id or mask");
  if (Q == 0) return HM_OK;                                              // nothing to score: no launch, nothing else is read
  if (!queries || !counts || !workspace) return hm_set_error(HM_ERR_ARG, "hm_mask_score: null queries, counts or workspace");
  if (workspace_bytes < hm_mask_score_workspace_bytes(Q, H, W, radius))
    return hm_set_error(HM_ERR_ARG, "hm_mask_score: workspace too small (hm_mask_score_workspace_bytes)");
  if (((uintptr_t)counts & 7) || ((uintptr_t)workspace & 7) || ((uintptr_t)pred_id & 3) || ((uintptr_t)queries & 3))
    return hm_set_error(HM_ERR_ARG, "hm_mask_score: counts and workspace must be 8-byte aligned, pred_id and queries 4-byte");
  MaskParams p;
  p.pred = pred_id; p.mask = mask; p.queries = queries;
  p.N = N; p.H = H; p.W = W; p.Q = Q; p.r = radius; p.words = (int)mask_words(W);
  p.counts = (unsigned long long*)counts; p.bits = (unsigned long long*)workspace;
  for (int d = 0; d <= MK_MAX_RADIUS; ++d) {
    int w = 0;
    if (d <= radius) while ((w + 1) * (w + 1) + d * d <= radius * radius) ++w;
    p.hw[d] = (uint8_t)w;
  }
  const long long strips = (H + MK_STRIP - 1) / MK_STRIP;
  const long long pack_blocks = ((long long)Q * strips * p.words + MK_WAVES - 1) / MK_WAVES;
  const long long chunks = ((long long)H * p.words + 63) / 64;
  const long long match_blocks = ((long long)Q * 2 * chunks + MK_WAVES - 1) / MK_WAVES;
  if (pack_blocks > 0x7fffffffll || match_blocks > 0x7fffffffll)
    return hm_set_error(HM_ERR_ARG, "hm_mask_score: Q * H * W too large for one call");
  hipStream_t s = (hipStream_t)stream_;
  HmProfScope prof(HM_K_OTHER, 2, Q, H, W, s);
  hipLaunchKernelGGL(mask_init_kernel, dim3((unsigned)(((long long)Q * 8 + MK_THREADS - 1) / MK_THREADS)), dim3(MK_THREADS), 0, s, p);
  int rc = hm_check_launch("hm_mask_score (init)");
  if (rc != HM_OK) return rc;
  hipLaunchKernelGGL(mask_pack_kernel, dim3((unsigned)pack_blocks), dim3(MK_THREADS), 0, s, p);
  rc = hm_check_launch("hm_mask_score (pack)");
  if (rc != HM_OK) return rc;
  hipLaunchKernelGGL(mask_match_kernel, dim3((unsigned)match_blocks), dim3(MK_THREADS), 0, s, p);
  return hm_check_launch("hm_mask_score (match)");
}
