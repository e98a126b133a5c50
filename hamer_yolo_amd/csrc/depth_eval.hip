// hm_depth_residuals - the predicted hands' z-buffer against a sensor depth map: per query a histogram of `sensor - predicted`
// over the pixels its meshes cover, six pixel counts, and the lower median, mean, mean absolute value and rms of the residuals
// (include/hamer_hip.h, "Depth residuals").
//
// The whole file is compiled without contraction (the pragma below) and every fp64 expression is written in the rule's order.
// The sums are integer atomics, so a query's histogram and counts depend on nothing but its own pixels and the scalars -- not
// on Q, N, the order of the meshes or the grid; stats is a function of that histogram and those counts alone.
//
// Three kernels on the stream, no host synchronisation, no allocation:
//   init   writes all of hist and counts (zeros) and the per-query range of occupied bins in the workspace (empty).
//   scan   ONE pass over the N * H * W pixels for all queries on depth_scan.h's walk, gate, query slots and groups of a wave
//          (shared with depth_fit.hip).  Covered pixels are added up in LDS before anything goes to memory: a workgroup keeps
//          DR_SLOTS queries, per query the six counts and a window of DR_WINDOW bins placed around the first residual it meets.
//          A pixel whose query found no slot, or whose bin lies outside its slot's window, adds straight to memory instead; both
//          ways add the same integers.  Within a group the counts are popcounts added by one lane, and so are the pixels of the
//          first two bins met, so a flat patch of one hand is a handful of LDS atomics and not 64 queued on one address.  At the
//          end the workgroup adds its non-zero LDS cells to memory, one atomic each, and the range of bins it touched.
//   stats  one wave per query: the occupied range of its histogram goes to LDS and lane 0 walks it in ascending order.
#include <math.h>
#include "common.h"
#include "depth_scan.h"

#pragma clang fp contract(off)

namespace {
using namespace depth_scan;

constexpr int DR_SLOTS = 4, DR_WINDOW = 512, DR_MAX_BINS = 4096;
enum { DR_BELOW = MEASURED, DR_ABOVE = 4, DR_IN_RANGE = 5 };  // the counts behind COVERED, OFF_MASK and NO_MEASUREMENT

struct DepthParams : Maps {
  int bins;
  double bin_m;
  unsigned int* hist;                                     // [Q][bins]
  unsigned long long* counts;                             // [Q][8]
  double* stats;                                          // [Q][4]
  int* range;                                             // workspace [Q][2]: the least and the greatest occupied bin
};

__global__ __launch_bounds__(THREADS) void depth_init_kernel(const DepthParams p) {
  const long long i = (long long)blockIdx.x * THREADS + threadIdx.x;
  if (i < (long long)p.Q * p.bins) p.hist[i] = 0u;
  if (i < (long long)p.Q * 8) p.counts[i] = 0ull;
  if (i < (long long)p.Q * 2) p.range[i] = (i & 1) ? -1 : 0x7fffffff;
}

struct DepthLds {
  unsigned int hist[DR_SLOTS][DR_WINDOW];
  unsigned int cnt[DR_SLOTS][8];
  int query[DR_SLOTS];                                    // q + 1 of the slot's query, 0 while it is free
  int base[DR_SLOTS];                                     // first bin of the slot's window, -1 until a residual placed it
  int lo[DR_SLOTS], hi[DR_SLOTS];                         // the range of non-zero window bins, found while they are added to memory
};

// what the rule makes of one pixel: its query (-1: the pixel is skipped), the count it ends in (OFF_MASK .. DR_IN_RANGE) and its bin
struct Pixel { int q, where, k; };

// one pixel by the rule of include/hamer_hip.h: e < total is its index, id its value of pred_id.  Nothing is added here.
__device__ __forceinline__ Pixel classify(const DepthParams& p, long long e, int id) {
  const Gate g = gate(p, (size_t)e, id);
  Pixel px = {g.q, g.stage, 0};
  if (g.q < 0 || g.stage != MEASURED) return px;
  const double r = (double)g.raw * p.unit - (double)p.depth[e];
  const double t = floor(r / p.bin_m);
  // |t| past 2^40 is outside every histogram; a NaN (of a NaN pred_depth, which the renderer never writes) counts as above
  px.where = DR_ABOVE;
  if (!(t < 1099511627776.0)) return px;
  px.where = DR_BELOW;
  if (t < -1099511627776.0) return px;
  const long long k = (long long)t + p.bins / 2;
  if (k < 0) return px;
  px.where = DR_ABOVE;
  if (k >= p.bins) return px;
  px.where = DR_IN_RANGE;
  px.k = (int)k;
  return px;
}

__device__ __forceinline__ void add_count(const DepthParams& p, DepthLds& s, int slot, int q, int which, int n) {
  if (n == 0) return;
  if (slot >= 0) atomicAdd(&s.cnt[slot][which], (unsigned int)n);
  else atomicAdd(p.counts + (size_t)q * 8 + which, (unsigned long long)n);
}

__device__ __forceinline__ void add_hist(const DepthParams& p, DepthLds& s, int slot, int base, int q, int k, int n) {
  const int j = k - base;
  if (slot >= 0 && base >= 0 && j >= 0 && j < DR_WINDOW) { atomicAdd(&s.hist[slot][j], (unsigned int)n); return; }
  atomicAdd(p.hist + (size_t)q * p.bins + (size_t)k, (unsigned int)n);
  // the range only ever widens within a call, so a plain read that already holds k spares the atomic (a stale read costs one)
  int* range = p.range + (size_t)q * 2;
  if (k < *(volatile int*)range) atomicMin(range, k);
  if (k > *(volatile int*)(range + 1)) atomicMax(range + 1, k);
}

// Adds one pixel per lane; the WHOLE wave calls this (depth_scan.h, for_each_query).  Neighbouring pixels often share a bin too:
// the lanes that share the first two bins met are counted with ballots and added by one lane, not queued 64 deep on one address.
__device__ __forceinline__ void tally(const DepthParams& p, DepthLds& s, const Pixel px, int lane) {
  for_each_query(px.q, [&](int leader, int q, bool mine, unsigned long long group) {
    int slot = -1, base = -1;
    const bool in_range = mine && px.where == DR_IN_RANGE;
    const unsigned long long placed = __ballot(in_range);
    const int k_first = placed ? __shfl(px.k, __ffsll((long long)placed) - 1) : 0;
    if (lane == leader) {
      slot = find_slot(s.query, q);
      if (slot >= 0) {
        base = *(volatile int*)&s.base[slot];
        if (base < 0 && placed) {                                         // the window goes around the first residual met
          int b = k_first - DR_WINDOW / 2;
          const int last = p.bins > DR_WINDOW ? p.bins - DR_WINDOW : 0;
          b = b < 0 ? 0 : b > last ? last : b;
          const int old = atomicCAS(&s.base[slot], -1, b);
          base = old < 0 ? b : old;
        }
      }
      add_count(p, s, slot, q, COVERED, __popcll(group));
      add_count(p, s, slot, q, DR_IN_RANGE, __popcll(placed));
    }
    slot = __shfl(slot, leader);
    base = __shfl(base, leader);
#pragma unroll
    for (int which = OFF_MASK; which <= DR_ABOVE; ++which) {
      const int n = __popcll(__ballot(mine && px.where == which));
      if (lane == leader) add_count(p, s, slot, q, which, n);
    }
    bool left = in_range;
#pragma unroll
    for (int turn = 0; turn < 2; ++turn) {
      const unsigned long long rest = __ballot(left);
      if (!rest) break;
      const int first = __ffsll((long long)rest) - 1;
      const int k = __shfl(px.k, first);
      const bool same = left && px.k == k;
      const int n = __popcll(__ballot(same));
      if (lane == first) add_hist(p, s, slot, base, q, k, n);
      left = left && !same;
    }
    if (left) add_hist(p, s, slot, base, q, px.k, 1);
  });
}

__global__ __launch_bounds__(THREADS) void depth_scan_kernel(const DepthParams p) {
  __shared__ DepthLds s;
  const int t = (int)threadIdx.x, lane = t & 63;
  for (int i = t; i < DR_SLOTS * DR_WINDOW; i += THREADS) (&s.hist[0][0])[i] = 0u;
  if (t < DR_SLOTS * 8) (&s.cnt[0][0])[t] = 0u;
  if (t < DR_SLOTS) { s.query[t] = 0; s.base[t] = -1; s.lo[t] = 0x7fffffff; s.hi[t] = -1; }
  __syncthreads();

  const Walk w = walk_of(p.id, p.total);
  for (int round = 0; round < ROUNDS; ++round) {
    int4 v[UNROLL];
    const long long e0 = load_round(w, round, t, v);
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const bool covered = (v[u].x & v[u].y & v[u].z & v[u].w) != -1;
      if (!__ballot(covered)) continue;                                                      // the wave's 256 pixels are uncovered
      const long long e = e0 + (long long)u * (4 * THREADS);
      tally(p, s, classify(p, e, v[u].x), lane); tally(p, s, classify(p, e + 1, v[u].y), lane);
      tally(p, s, classify(p, e + 2, v[u].z), lane); tally(p, s, classify(p, e + 3, v[u].w), lane);
    }
  }
  scan_edges(w, p.id, t, [&](long long e, int id) { tally(p, s, classify(p, e, id), lane); });
  __syncthreads();

  // what the workgroup gathered goes to memory: one atomic per non-zero cell
  for (int i = t; i < DR_SLOTS * DR_WINDOW; i += THREADS) {
    const unsigned int n = (&s.hist[0][0])[i];
    if (n == 0u) continue;
    const int slot = i / DR_WINDOW, k = s.base[slot] + (i - slot * DR_WINDOW);
    atomicAdd(p.hist + (size_t)(s.query[slot] - 1) * p.bins + (size_t)k, n);
    atomicMin(&s.lo[slot], k);
    atomicMax(&s.hi[slot], k);
  }
  if (t < DR_SLOTS * 8) {
    const unsigned int n = (&s.cnt[0][0])[t];
    if (n != 0u) atomicAdd(p.counts + (size_t)(s.query[t >> 3] - 1) * 8 + (t & 7), (unsigned long long)n);
  }
  __syncthreads();
  if (t < DR_SLOTS && s.hi[t] >= 0) {
    atomicMin(p.range + (size_t)(s.query[t] - 1) * 2, s.lo[t]);
    atomicMax(p.range + (size_t)(s.query[t] - 1) * 2 + 1, s.hi[t]);
  }
}

__global__ __launch_bounds__(64) void depth_stats_kernel(const DepthParams p) {
  __shared__ unsigned int h[DR_MAX_BINS];
  const int q = (int)blockIdx.x, lane = (int)threadIdx.x;
  int lo = p.range[(size_t)q * 2], hi = p.range[(size_t)q * 2 + 1];
  if (hi < lo || lo < 0 || hi >= p.bins) { lo = 0; hi = -1; }                                // no pixel in range: nothing is read
  for (int k = lo + lane; k <= hi; k += 64) h[k - lo] = p.hist[(size_t)q * p.bins + k];
  __syncthreads();
  if (lane != 0) return;
  const unsigned long long* c = p.counts + (size_t)q * 8;
  const unsigned long long below = c[DR_BELOW], above = c[DR_ABOVE], inside = c[DR_IN_RANGE];
  const unsigned long long n = below + inside + above, m = (n + 1) / 2;
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  const bool find = n > 0 && m > below && m <= below + inside;
  double median = nan, s1 = 0.0, s2 = 0.0, s3 = 0.0;
  unsigned long long cum = below;
  bool found = false;
  for (int k = lo; k <= hi; ++k) {
    const unsigned int cnt = h[k - lo];
    if (cnt == 0u) continue;
    const double centre = ((double)(k - p.bins / 2) + 0.5) * p.bin_m;
    const double w = (double)cnt;
    s1 = s1 + w * centre;
    s2 = s2 + w * fabs(centre);
    s3 = s3 + w * (centre * centre);
    cum += cnt;
    if (find && !found && cum >= m) { median = centre; found = true; }
  }
  double* out = p.stats + (size_t)q * 4;
  out[0] = median;
  if (inside == 0) { out[1] = nan; out[2] = nan; out[3] = nan; return; }
  const double d = (double)inside;
  out[1] = s1 / d;
  out[2] = s2 / d;
  out[3] = sqrt(s3 / d);
}

}  // namespace

extern "C" size_t hm_depth_residuals_workspace_bytes(int Q, int bins) {
  if (Q < 0 || bins < 2 || bins > DR_MAX_BINS || (bins & 1)) return 0;
  return (size_t)(Q < 1 ? 1 : Q) * 2 * sizeof(int);                        // never 0 for legal sizes: Q == 0 asks for one query's
}

extern "C" int hm_depth_residuals(const float* pred_depth, const int32_t* pred_id, const uint16_t* sensor, const uint8_t* mask,
                                  const int32_t* labels, int N, int H, int W, const int32_t* mesh_query, int n_meshes, int Q,
                                  double unit, int raw_lo, int raw_hi, double bin_m, int bins, uint32_t* hist, int64_t* counts,
                                  double* stats, void* workspace, size_t workspace_bytes, void* stream_) {
  DepthParams p;
  p.depth = pred_depth; p.id = pred_id; p.sensor = sensor; p.mask = mask; p.labels = labels; p.mesh_query = mesh_query;
  p.n_meshes = n_meshes; p.Q = Q; p.bins = bins; p.raw_lo = raw_lo; p.raw_hi = raw_hi; p.unit = unit; p.bin_m = bin_m;
  p.hist = hist; p.counts = (unsigned long long*)counts; p.stats = stats; p.range = (int*)workspace;
  const char* scalars = (bins < 2 || bins > DR_MAX_BINS || (bins & 1)) ? "bins must be even and in 2..4096"
      : (!positive_finite(unit) || !positive_finite(bin_m))            ? "unit and bin_m must be finite numbers > 0" : nullptr;
  const char* buffers = ((n_meshes > 0 && !mesh_query) || !hist || !counts || !stats || !workspace)
          ? "null mesh_query, hist, counts, stats or workspace"
      : workspace_bytes < hm_depth_residuals_workspace_bytes(Q, bins) ? "workspace too small (hm_depth_residuals_workspace_bytes)"
      : (((uintptr_t)counts & 7) || ((uintptr_t)stats & 7) || ((uintptr_t)hist & 3) || ((uintptr_t)workspace & 3))
          ? "counts and stats must be 8-byte aligned, hist and workspace 4-byte" : nullptr;
  int rc = host_checks("hm_depth_residuals", p, N, H, W, scalars, nullptr, buffers);
  if (rc != HM_OK || Q == 0) return rc;                                  // no query, nothing to score: no launch
  const long long cells = (long long)Q * bins > (long long)Q * 8 ? (long long)Q * bins : (long long)Q * 8;
  const long long init_blocks = (cells + THREADS - 1) / THREADS;
  if (init_blocks > 0x7fffffffll) return hm_set_error(HM_ERR_ARG, "hm_depth_residuals: Q * bins too large for one call");
  hipStream_t s = (hipStream_t)stream_;
  HmProfScope prof(HM_K_OTHER, 8, Q, H, W, s);
  hipLaunchKernelGGL(depth_init_kernel, dim3((unsigned)init_blocks), dim3(THREADS), 0, s, p);
  rc = hm_check_launch("hm_depth_residuals (init)");
  if (rc != HM_OK) return rc;
  hipLaunchKernelGGL(depth_scan_kernel, dim3(scan_blocks(p.total)), dim3(THREADS), 0, s, p);
  rc = hm_check_launch("hm_depth_residuals (scan)");
  if (rc != HM_OK) return rc;
  hipLaunchKernelGGL(depth_stats_kernel, dim3((unsigned)Q), dim3(64), 0, s, p);
  return hm_check_launch("hm_depth_residuals (stats)");
}
