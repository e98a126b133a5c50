// The boundary pack of the mask path, shared by mask_eval.hip and mask_fit.hip: both entry points
// turn a query's two images into the same pair of boundary maps, one bit per pixel, before they match them in their own ways.
// Integer and bit arithmetic only, like depth_scan.h.
// The pack: one wave per (query, strip of 32 rows, 64-pixel word of a row).  Lane l reads pixel x = 64 c + l (clamped to W - 1:
// the replicated last column) of one row; __ballot turns the wave's 64 answers into one word of the pred image and one of the
// gt image.  Lane 63 also reads pixel 64 c + 64 (clamped), the east neighbour of the word's last pixel.  With the word of the
// next row (clamped to H - 1: the replicated last row) the boundary map is three XORs of whole words:
//   b = ((s ^ east(s)) | (s ^ south) | (s ^ east(south))) & valid,   east(w) = (w >> 1) | (extra << 63).
// The two boundary words go to the workspace ([Q][2][H][ceil(W / 64)] uint64, bits at or past W are zero).  The south rows of 8
// rows are loaded before any is used, so a wave has 16 row loads in flight.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include "hamer_hip_internal.h"

namespace mask_bits {

constexpr int MAX_RADIUS = 64, STRIP = 32, GROUP = 8, THREADS = 256, WAVES = THREADS / 64;

// What both entry points' kernels take; a kernel's parameters derive from this.
struct Params {
  const int32_t* pred; const uint8_t* mask; const hm_mask_query* queries;
  int N, H, W, Q, r, words;                              // words = ceil(W / 64)
  unsigned long long* bits;                              // [Q][2][H][words]
  uint8_t hw[MAX_RADIUS + 1];                            // hw[d] = floor(sqrt(r r - d d)) for d <= r
};

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

// A pack kernel: the wave's task, its strip row by row, the two stores.  row(cur, bpw, bgw, valid) sees every row of the strip
// once, wave-uniformly: the row's own words, its two boundary words and the mask of the word's pixels inside the image.
// Returns the wave's query, or -1 when the wave has no task or its query's frame lies outside the batch (a whole wave
// leaves: nothing here synchronises).
template <class Row>
__device__ __forceinline__ int pack_strips(const Params& p, Row&& row) {
  const int lane = threadIdx.x & 63, H = p.H, W = p.W, words = p.words;
  const bool last_lane = lane == 63;
  const int strips = (H + STRIP - 1) / STRIP;
  const long long per_query = (long long)strips * words;
  const long long task = (long long)blockIdx.x * WAVES + (threadIdx.x >> 6);
  if (task >= per_query * p.Q) return -1;
  const int q = (int)(task / per_query);
  const int rem = (int)(task - (long long)q * per_query);
  const int strip = rem / words, c = rem - strip * words;
  const hm_mask_query qu = p.queries[q];
  if (qu.frame < 0 || qu.frame >= p.N) return -1;
  const int x = c * 64 + lane;
  const int xc = x < W ? x : W - 1, xe = c * 64 + 64 < W ? c * 64 + 64 : W - 1;
  const unsigned long long valid = __ballot(x < W);
  const size_t plane = (size_t)H * (size_t)W;
  const int32_t* __restrict__ pr = p.pred + (size_t)qu.frame * plane;
  const uint8_t* __restrict__ mk = p.mask + (size_t)qu.frame * plane;
  unsigned long long* __restrict__ bp = p.bits + ((size_t)q * 2 + 0) * (size_t)H * words;
  unsigned long long* __restrict__ bg = p.bits + ((size_t)q * 2 + 1) * (size_t)H * words;
  const int y0 = strip * STRIP, y_end = y0 + STRIP < H ? y0 + STRIP : H;
  RowWords cur = row_words(load_row(pr + (size_t)y0 * W, mk + (size_t)y0 * W, xc, xe, last_lane), last_lane, qu.id_lo, qu.id_hi, qu.label);
  for (int yb = y0; yb < y_end; yb += GROUP) {
    // the south rows of GROUP rows are read before any is used: the loads of a group are in flight together.  A row index is
    // clamped to H - 1, so the last row's south neighbour is itself and no load leaves the image
    RowPixels south[GROUP];
#pragma unroll
    for (int k = 0; k < GROUP; ++k) {
      const int ys = yb + 1 + k < H ? yb + 1 + k : H - 1;
      south[k] = load_row(pr + (size_t)ys * W, mk + (size_t)ys * W, xc, xe, last_lane);
    }
#pragma unroll
    for (int k = 0; k < GROUP; ++k) {
      const int y = yb + k;
      if (y >= y_end) break;
      const RowWords nxt = row_words(south[k], last_lane, qu.id_lo, qu.id_hi, qu.label);
      const unsigned long long pe = (cur.p >> 1) | cur.ep, pse = (nxt.p >> 1) | nxt.ep;
      const unsigned long long ge = (cur.g >> 1) | cur.eg, gse = (nxt.g >> 1) | nxt.eg;
      const unsigned long long bpw = ((cur.p ^ pe) | (cur.p ^ nxt.p) | (cur.p ^ pse)) & valid;
      const unsigned long long bgw = ((cur.g ^ ge) | (cur.g ^ nxt.g) | (cur.g ^ gse)) & valid;
      if (lane == 0) {
        bp[(size_t)y * words + c] = bpw;
        bg[(size_t)y * words + c] = bgw;
      }
      row(cur, bpw, bgw, valid);
      cur = nxt;
    }
  }
  return q;
}

// ---------------------------------------------------------------------------------------------------------------- host side
inline long long words_of(int W) { return ((long long)W + 63) / 64; }
// The uint64 words of the boundary maps of Q queries.
inline size_t map_words(int Q, int H, int W) { return (size_t)Q * 2 * (size_t)H * (size_t)words_of(W); }
inline long long pack_blocks(const Params& p) { return ((long long)p.Q * ((p.H + STRIP - 1) / STRIP) * p.words + WAVES - 1) / WAVES; }

// The checks both entry points (`name`) make of the arguments in p, in the one order their callers see; on success p.words and
// the half-width table p.hw are set.  An entry point's own complaints are ranked among them and come as the text behind "name: ", or null: scalars
// about its other scalars, buffers about its own pointers and workspace -- not looked at with Q == 0: HM_OK, no launch,
// nothing else is read.
inline int host_checks(const char* name, Params& p, const char* scalars, const char* buffers) {
  char msg[192];
  auto fail = [&](const char* text) { snprintf(msg, sizeof(msg), "%s: %s", name, text); return hm_set_error(HM_ERR_ARG, msg); };
  if (p.N < 1 || p.H < 1 || p.W < 1) return fail("N, H and W must be positive");
  if ((long long)p.N * p.H * p.W >= (1ll << 31)) return fail("N * H * W must be below 2^31");
  if (p.r < 0 || p.r > MAX_RADIUS) return fail("radius must be in 0..64");
  if (scalars) return fail(scalars);
  if (p.Q < 0) return fail("Q must not be negative");
  if (!p.pred || !p.mask) return fail("null pred_id or mask");
  if (p.Q == 0) return HM_OK;
  if (buffers) return fail(buffers);
  p.words = (int)words_of(p.W);
  for (int d = 0; d <= MAX_RADIUS; ++d) {
    int w = 0;
    if (d <= p.r) while ((w + 1) * (w + 1) + d * d <= p.r * p.r) ++w;
    p.hw[d] = (uint8_t)w;
  }
  return HM_OK;
}

}  // namespace mask_bits
