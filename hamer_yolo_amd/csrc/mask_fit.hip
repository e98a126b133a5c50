// hm_mask_fit - the 2-D similarity (image-plane shift, scale, rotation about the viewing axis) that brings a predicted
// silhouette's contour onto a label mask's: per query the 4 x 4 normal equations of a contour alignment, ten pixel counts and
// their damped Cholesky solution (include/hamer_hip.h, "Mask fit").
//
// All per-pixel work is integer; the only fp64 of the match pass is one correctly rounded division per term, rounded to an
// integer (llrint of the quotient times 2^20) before it is added.  The sums are integer atomics, so a query's sums and counts
// depend on nothing but its own two images and the scalars -- not on Q, the order of the queries, the rest of the batch or the
// grid; solution is a function of those integers and the scalars alone.  The solve is fp64 with contraction off (the pragma
// below) and every expression is written in the rule's order.
//
// Four kernels on the stream, no host synchronisation, no allocation.  The workspace holds the boundary maps, [Q][2][H]
// [ceil(W / 64)] uint64 with one bit per pixel (mask_bits.h, shared with mask_eval.hip; bits at or past W are zero), followed by
// one row of 32 int64 per query where the sums are added up: 18 sums, 2 x 6 counts, 2 unused.
//   init   zeroes the rows of sums and counts.  The boundary maps need no clearing: pack writes every word of every query whose
//          frame is inside the batch, and the maps of the other queries are never read.
//   pack   the boundary pack of mask_bits.h and nothing else.
//   match  one workgroup per (query, direction, tile of 32 rows x one 64-pixel word) of the direction's OWN boundary map.  A tile
//          without a boundary pixel -- nearly all of them -- costs one load per row.  Otherwise the 32 + 2 r rows x 3 words of the
//          OTHER map that the tile's discs can reach go to LDS, the tile's set bits are compacted into a queue in LDS (a row's
//          word is its own ballot; a bit's slot is the popcount prefix of the rows before it plus that of the bits below it),
//          and the lanes take queue entries, not pixels: every lane of every wave but the last has a boundary pixel.  A lane
//          walks the rows |dy| = 0, 1, 1, 2, 2 .. while dy dy <= the best d2 so far; per row the chord's nearest set bit left
//          and right of the pixel's column comes from a clz and a ctz of two 64-bit windows cut from the row's three words.
//          Each of the 18 terms is added across the wave with 64-bit shuffles (integer adds commute, so the tree is exact), the
//          five counts are popcounts of ballots, and lane 0 adds what is not zero ONCE per wave to the workgroup's row in LDS;
//          at the end the workgroup sends one 64-bit atomic per non-zero cell to the query's row.
//   solve  one thread per query: copies its row to sums and counts, builds M, factorises and solves in the header's order.
#include <limits.h>
#include <math.h>
#include "common.h"
#include "mask_bits.h"

#pragma clang fp contract(off)

namespace {
using namespace mask_bits;

constexpr int MF_MAX_REACH = 4096;
constexpr int MF_TILE = 32;                               // rows of a match tile
constexpr int MF_ROWS = MF_TILE + 2 * MAX_RADIUS;         // rows of the other map a tile can reach
constexpr int MF_SUMS = 18, MF_COUNTS = 12, MF_CELLS = 32;
constexpr int MF_LOCAL = MF_SUMS + 5;                     // what a workgroup gathers: the sums and its direction's five counts
constexpr double MF_SCALE = 1048576.0, MF_INV_SCALE = 1.0 / 1048576.0;        // 2^20 and 2^-20: exact
enum { MF_NONE = 0, MF_LINE = 1, MF_ANCHOR = 2, MF_UNMATCHED = 3, MF_OUT = 4 };

struct MaskFitParams : Params {
  const int32_t* centre;
  int reach, directions, min_pixels, tiles;               // tiles = ceil(H / MF_TILE)
  double damping, lever2;
  unsigned long long* acc;                                // [Q][32]
  long long* sums;                                        // [Q][18]
  long long* counts;                                      // [Q][2][6]
  double* solution;                                       // [Q][8]
};

__global__ __launch_bounds__(THREADS) void mfit_init_kernel(const MaskFitParams p) {
  const long long i = (long long)blockIdx.x * THREADS + threadIdx.x;
  if (i < (long long)p.Q * MF_CELLS) p.acc[i] = 0ull;
}

// ------------------------------------------------------------------------------------------------------------------ pack
__global__ __launch_bounds__(THREADS) void mfit_pack_kernel(const MaskFitParams p) {
  pack_strips(p, [](const RowWords&, unsigned long long, unsigned long long, unsigned long long) {});
}

// ----------------------------------------------------------------------------------------------------------------- match
struct MatchLds {
  unsigned long long other[MF_ROWS][3];                   // the other map: rows y0 - r .. y0 + 31 + r, words c - 1 .. c + 1
  unsigned long long mine[MF_TILE];                       // the tile's own words
  unsigned long long acc[MF_LOCAL + 1];
  int base[MF_TILE + 1];                                  // set bits in the rows before a row
  unsigned short queue[MF_TILE * 64];                     // row << 6 | bit of every boundary pixel of the tile, row-major
  uint8_t hw[MAX_RADIUS + 1];
};

__device__ __forceinline__ long long wave_sum(long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

__device__ __forceinline__ void add_local(MatchLds& s, int cell, long long n) {
  if (n != 0) __hip_atomic_fetch_add(&s.acc[cell], (unsigned long long)n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// The set bit of the row (lo : mid : hi, ascending x) nearest to bit `bit` of mid within w pixels, 0 <= w <= 64; on a tie the one
// on the left.  Returns false when there is none.
__device__ __forceinline__ bool nearest_in_row(unsigned long long lo, unsigned long long mid, unsigned long long hi, int bit, int w, int& dx) {
  if ((mid >> bit) & 1ull) { dx = 0; return true; }
  if (w == 0) return false;
  // left: the 64 pixels before the column, the nearest in bit 63;  right: the 64 pixels after it, the nearest in bit 0
  unsigned long long left = bit == 0 ? lo : (lo >> bit) | (mid << (64 - bit));
  unsigned long long right = bit == 63 ? hi : (mid >> (bit + 1)) | (hi << (63 - bit));
  if (w < 64) { left &= ~0ull << (64 - w); right &= (1ull << w) - 1ull; }
  const int l = left ? __clzll((long long)left) + 1 : 1000, rr = right ? __ffsll((long long)right) : 1000;
  if (l == 1000 && rr == 1000) return false;
  dx = l <= rr ? -l : rr;
  return true;
}

__global__ __launch_bounds__(THREADS) void mfit_match_kernel(const MaskFitParams p) {
  __shared__ MatchLds s;
  const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
  long long b = (long long)blockIdx.x;
  const int c = (int)(b % p.words); b /= p.words;
  const int tile = (int)(b % p.tiles); b /= p.tiles;
  const int side = (int)(b & 1), q = (int)(b >> 1);
  if (!((p.directions >> side) & 1)) return;                            // every return before the first barrier is the workgroup's
  const int frame = p.queries[q].frame;
  if (frame < 0 || frame >= p.N) return;
  const size_t items = (size_t)p.H * (size_t)p.words;
  const unsigned long long* __restrict__ mine = p.bits + ((size_t)q * 2 + side) * items;
  const unsigned long long* __restrict__ other = p.bits + ((size_t)q * 2 + (1 - side)) * items;
  const int y0 = tile * MF_TILE, r = p.r;
  if (t < MF_TILE) s.mine[t] = y0 + t < p.H ? mine[(size_t)(y0 + t) * p.words + c] : 0ull;
  if (t <= MF_LOCAL) s.acc[t] = 0ull;
  if (t <= MAX_RADIUS) s.hw[t] = p.hw[t];
  __syncthreads();
  unsigned long long any = 0ull;
#pragma unroll
  for (int i = 0; i < MF_TILE; ++i) any |= s.mine[i];
  if (any == 0ull) return;                                              // the same for every thread: no boundary pixel in the tile

  const int rows = MF_TILE + 2 * r;
  for (int i = t; i < rows * 3; i += THREADS) {
    const int rr = i / 3, k = i - rr * 3;
    const int yy = y0 - r + rr, cc = c - 1 + k;
    s.other[rr][k] = (yy >= 0 && yy < p.H && cc >= 0 && cc < p.words) ? other[(size_t)yy * p.words + cc] : 0ull;
  }
  if (t <= MF_TILE) {
    int n = 0;
    for (int i = 0; i < t; ++i) n += __popcll(s.mine[i]);
    s.base[t] = n;
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < MF_TILE / WAVES; ++i) {
    const int row = i * WAVES + wave;
    const unsigned long long a = s.mine[row];
    if ((a >> lane) & 1ull) s.queue[s.base[row] + __popcll(a & ((1ull << lane) - 1ull))] = (unsigned short)((row << 6) | lane);
  }
  __syncthreads();
  const int total = s.base[MF_TILE];
  const long long cx = (long long)p.centre[(size_t)q * 2], cy = (long long)p.centre[(size_t)q * 2 + 1];
  const long long reach = (long long)p.reach, reach2 = reach * reach;

  for (int e0 = wave * 64; e0 < total; e0 += THREADS) {              // wave-uniform: the whole wave shuffles below
    const bool active = e0 + lane < total;
    int where = MF_NONE, best = INT_MAX, bdx = 0, bdy = 0, row = 0, bit = 0;
    if (active) {
      const int code = (int)s.queue[e0 + lane];
      row = code >> 6; bit = code & 63;
      for (int k = 0; k <= r && k * k <= best; ++k) {
        const int w = (int)s.hw[k];
#pragma unroll
        for (int sg = 0; sg < 2; ++sg) {
          if (sg == 1 && k == 0) break;
          const int dy = sg == 0 ? -k : k;
          const unsigned long long* rw = s.other[row + dy + r];
          const unsigned long long lo = rw[0], mid = rw[1], hi = rw[2];
          int dx;
          if ((lo | mid | hi) == 0ull || !nearest_in_row(lo, mid, hi, bit, w, dx)) continue;
          const int d2 = dx * dx + k * k;
          if (d2 < best || (d2 == best && dy < bdy)) { best = d2; bdx = dx; bdy = dy; }
        }
      }
      where = MF_UNMATCHED;
    }
    long long ux = 0, uy = 0, ddx = 0, ddy = 0;
    if (active && best != INT_MAX) {
      const long long x = (long long)c * 64 + bit, y = (long long)y0 + row;
      if (side == 0) { ux = x - cx; uy = y - cy; ddx = bdx; ddy = bdy; }
      else { ux = x + bdx - cx; uy = y + bdy - cy; ddx = -bdx; ddy = -bdy; }
      const bool near = ux >= -reach && ux <= reach && uy >= -reach && uy <= reach;      // so that the squares cannot overflow
      where = !(near && ux * ux + uy * uy <= reach2) ? MF_OUT : best > 0 ? MF_LINE : MF_ANCHOR;
    }
    {
      const int n_all = __popcll(__ballot(active)), n_line = __popcll(__ballot(where == MF_LINE));
      const int n_anchor = __popcll(__ballot(where == MF_ANCHOR)), n_un = __popcll(__ballot(where == MF_UNMATCHED));
      const int n_out = __popcll(__ballot(where == MF_OUT));
      if (lane == 0) {
        add_local(s, MF_SUMS + 0, n_all); add_local(s, MF_SUMS + 1, n_line); add_local(s, MF_SUMS + 2, n_anchor);
        add_local(s, MF_SUMS + 3, n_un); add_local(s, MF_SUMS + 4, n_out);
      }
    }
    const bool line = where == MF_LINE, anchor = where == MF_ANCHOR;
    if (__ballot(line)) {
      long long J[4];
      J[0] = ddx * ux + ddy * uy; J[1] = ddy * ux - ddx * uy; J[2] = ddx; J[3] = ddy;
      const double d2 = (double)(line ? best : 1);
      int cell = 0;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int j = i; j < 4; ++j) {
          const long long v = wave_sum(line ? llrint((double)(J[i] * J[j]) / d2 * MF_SCALE) : 0ll);
          if (lane == 0) add_local(s, cell, v);
          ++cell;
        }
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const long long v = wave_sum(line ? J[i] : 0ll);
        if (lane == 0) add_local(s, 10 + i, v);
      }
      const long long v = wave_sum(line ? (long long)best : 0ll);
      if (lane == 0) add_local(s, 14, v);
    }
    if (__ballot(anchor)) {
      const long long sx = wave_sum(anchor ? ux : 0ll), sy = wave_sum(anchor ? uy : 0ll), su = wave_sum(anchor ? ux * ux + uy * uy : 0ll);
      if (lane == 0) { add_local(s, 15, sx); add_local(s, 16, sy); add_local(s, 17, su); }
    }
  }
  __syncthreads();
  if (t < MF_LOCAL) {
    const unsigned long long n = s.acc[t];
    const int cell = t < MF_SUMS ? t : MF_SUMS + side * 6 + (t - MF_SUMS);
    if (n != 0ull) atomicAdd(p.acc + (size_t)q * MF_CELLS + cell, n);
  }
}

// ----------------------------------------------------------------------------------------------------------------- solve
__global__ __launch_bounds__(64) void mfit_solve_kernel(const MaskFitParams p) {
  const int q = (int)blockIdx.x * 64 + (int)threadIdx.x;
  if (q >= p.Q) return;
  const unsigned long long* row = p.acc + (size_t)q * MF_CELLS;
  long long sum[MF_SUMS], cnt[MF_COUNTS];
#pragma unroll
  for (int i = 0; i < MF_SUMS; ++i) { sum[i] = (long long)row[i]; p.sums[(size_t)q * MF_SUMS + i] = sum[i]; }
#pragma unroll
  for (int i = 0; i < MF_COUNTS; ++i) { cnt[i] = (long long)row[MF_SUMS + i]; p.counts[(size_t)q * MF_COUNTS + i] = cnt[i]; }
  const long long used = cnt[1] + cnt[2] + cnt[7] + cnt[8];

  double M[4][4], g[4];
  {
    int k = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
      for (int j = i; j < 4; ++j) { M[i][j] = (double)sum[k] * MF_INV_SCALE; ++k; }
    }
  }
  const double na = (double)(cnt[2] + cnt[8]), sx = (double)sum[15], sy = (double)sum[16], suu = (double)sum[17];
  M[0][0] = M[0][0] + suu; M[1][1] = M[1][1] + suu;
  M[0][2] = M[0][2] + sx;  M[0][3] = M[0][3] + sy;
  M[1][2] = M[1][2] - sy;  M[1][3] = M[1][3] + sx;
  M[2][2] = M[2][2] + na;  M[3][3] = M[3][3] + na;
  const double du = p.damping * (double)used;
  M[0][0] = M[0][0] + du * p.lever2; M[1][1] = M[1][1] + du * p.lever2;
  M[2][2] = M[2][2] + du;            M[3][3] = M[3][3] + du;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
#pragma unroll
    for (int j = 0; j < i; ++j) M[i][j] = M[j][i];
    g[i] = (double)sum[10 + i];
  }

  // Cholesky M = L L^T, column by column, every inner sum from k = 0 upwards
  double Lm[4][4];
  bool ok = used >= (long long)p.min_pixels;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    double sj = M[j][j];
#pragma unroll
    for (int k = 0; k < j; ++k) sj = sj - Lm[j][k] * Lm[j][k];
    if (!(sj > 0.0)) ok = false;
    Lm[j][j] = sqrt(sj);
#pragma unroll
    for (int i = j + 1; i < 4; ++i) {
      double sij = M[i][j];
#pragma unroll
      for (int k = 0; k < j; ++k) sij = sij - Lm[i][k] * Lm[j][k];
      Lm[i][j] = sij / Lm[j][j];
    }
  }
  double y[4], x[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    double si = g[i];
#pragma unroll
    for (int k = 0; k < i; ++k) si = si - Lm[i][k] * y[k];
    y[i] = si / Lm[i][i];
  }
#pragma unroll
  for (int i = 3; i >= 0; --i) {
    double si = y[i];
#pragma unroll
    for (int k = i + 1; k < 4; ++k) si = si - Lm[k][i] * x[k];
    x[i] = si / Lm[i][i];
  }
  double* out = p.solution + (size_t)q * 8;
#pragma unroll
  for (int i = 0; i < 4; ++i) out[i] = ok ? x[i] : 0.0;
  out[4] = used > 0 ? sqrt((double)sum[14] / (double)used) : 0.0;
  out[5] = ok ? 1.0 : 0.0;
  out[6] = 0.0; out[7] = 0.0;
}

}  // namespace

extern "C" size_t hm_mask_fit_workspace_bytes(int Q, int H, int W, int radius) {
  if (Q < 0 || H < 1 || W < 1 || radius < 0 || radius > MAX_RADIUS) return 0;
  const size_t n = (size_t)(Q < 1 ? 1 : Q);                              // never 0 for legal sizes: Q == 0 asks for one query's
  return (map_words((int)n, H, W) + n * MF_CELLS) * sizeof(unsigned long long);
}

extern "C" int hm_mask_fit(const int32_t* pred_id, const uint8_t* mask, int N, int H, int W, const hm_mask_query* queries, int Q,
                           const int32_t* centre, int radius, int reach_px, int directions, double damping, double lever_px,
                           int min_pixels, int64_t* sums, int64_t* counts, double* solution, void* workspace,
                           size_t workspace_bytes, void* stream_) {
  MaskFitParams p;
  p.pred = pred_id; p.mask = mask; p.queries = queries; p.centre = centre;
  p.N = N; p.H = H; p.W = W; p.Q = Q; p.r = radius; p.reach = reach_px; p.directions = directions;
  p.min_pixels = min_pixels; p.damping = damping; p.lever2 = lever_px * lever_px;
  p.bits = (unsigned long long*)workspace;
  p.sums = (long long*)sums; p.counts = (long long*)counts; p.solution = solution;
  const char* scalars = (reach_px < 1 || reach_px > MF_MAX_REACH) ? "reach_px must be in 1..4096"
      : (directions < 1 || directions > 3)        ? "directions must be 1, 2 or 3"
      : !(damping >= 0.0 && damping < INFINITY)   ? "damping must be a finite number >= 0"
      : !positive_finite(lever_px)                ? "lever_px must be a finite number > 0"
      : min_pixels < 1                            ? "min_pixels must be at least 1" : nullptr;
  const char* buffers = (!queries || !centre || !sums || !counts || !solution || !workspace)
          ? "null queries, centre, sums, counts, solution or workspace"
      : workspace_bytes < hm_mask_fit_workspace_bytes(Q, H, W, radius) ? "workspace too small (hm_mask_fit_workspace_bytes)"
      : (((uintptr_t)sums & 7) || ((uintptr_t)counts & 7) || ((uintptr_t)solution & 7) || ((uintptr_t)workspace & 7) ||
         ((uintptr_t)pred_id & 3) || ((uintptr_t)queries & 3) || ((uintptr_t)centre & 3))
          ? "sums, counts, solution and workspace must be 8-byte aligned, pred_id, queries and centre 4-byte" : nullptr;
  int rc = host_checks("hm_mask_fit", p, scalars, buffers);
  if (rc != HM_OK || Q == 0) return rc;                                  // no query, nothing to fit: no launch
  p.tiles = (H + MF_TILE - 1) / MF_TILE;
  p.acc = p.bits + map_words(Q, H, W);
  const long long match_blocks = (long long)Q * 2 * p.tiles * p.words;
  if (pack_blocks(p) > 0x7fffffffll || match_blocks > 0x7fffffffll)
    return hm_set_error(HM_ERR_ARG, "hm_mask_fit: Q * H * W too large for one call");
  hipStream_t s = (hipStream_t)stream_;
  HmProfScope prof(HM_K_OTHER, 10, Q, H, W, s);
  hipLaunchKernelGGL(mfit_init_kernel, dim3((unsigned)(((long long)Q * MF_CELLS + THREADS - 1) / THREADS)), dim3(THREADS), 0, s, p);
  rc = hm_check_launch("hm_mask_fit (init)");
  if (rc != HM_OK) return rc;
  hipLaunchKernelGGL(mfit_pack_kernel, dim3((unsigned)pack_blocks(p)), dim3(THREADS), 0, s, p);
  rc = hm_check_launch("hm_mask_fit (pack)");
  if (rc != HM_OK) return rc;
  hipLaunchKernelGGL(mfit_match_kernel, dim3((unsigned)match_blocks), dim3(THREADS), 0, s, p);
  rc = hm_check_launch("hm_mask_fit (match)");
  if (rc != HM_OK) return rc;
  hipLaunchKernelGGL(mfit_solve_kernel, dim3((unsigned)((Q + 63) / 64)), dim3(64), 0, s, p);
  return hm_check_launch("hm_mask_fit (solve)");
}
