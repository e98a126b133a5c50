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
//   scan   ONE pass over the N * H * W pixels for all queries.  The pixels are walked as consecutive int32 of pred_id, not row
//          by row: from the first 16-byte aligned address on, a thread reads four 16-byte vectors per round (all four loads are
//          issued before any is looked at) and a workgroup of 256 threads does DR_ROUNDS rounds, 32768 pixels; the up to 3
//          pixels before the first aligned address and behind the last whole vector are read one by one by the first
//          workgroup.  A vector of four -1 -- nearly all of them -- costs that load: pred_depth, sensor and mask are read for
//          covered pixels only.  Covered pixels are added up in LDS before anything goes to memory: a workgroup keeps
//          DR_SLOTS queries (claimed first come, first served), per query the six counts and a window of DR_WINDOW bins placed
//          around the first residual it meets.  A pixel whose query found no slot, or whose bin lies outside its slot's window,
//          adds straight to memory instead; both ways add the same integers.  Within a wave the 64 pixels of a step are first
//          grouped by query with ballots: the counts of a group are popcounts added by one lane, and so are the pixels of the
//          first two bins met, so a flat patch of one hand is a handful of LDS atomics and not 64 queued on one address.  At
//          the end the workgroup adds its non-zero LDS cells to memory, one atomic each, and the range of bins it touched.
//   stats  one wave per query: the occupied range of its histogram goes to LDS and lane 0 walks it in ascending order.
#include <math.h>
#include <stdint.h>
#include "common.h"
#include "hamer_hip_internal.h"

#pragma clang fp contract(off)

namespace {

constexpr int DR_THREADS = 256, DR_UNROLL = 4, DR_ROUNDS = 8, DR_SLOTS = 4, DR_WINDOW = 512, DR_MAX_BINS = 4096;
constexpr long long DR_VECS = (long long)DR_THREADS * DR_UNROLL * DR_ROUNDS;      // 16-byte vectors per workgroup: 32768 pixels
enum { DR_COVERED = 0, DR_OFF_MASK = 1, DR_NO_MEASUREMENT = 2, DR_BELOW = 3, DR_ABOVE = 4, DR_IN_RANGE = 5 };

struct DepthParams {
  const float* depth; const int32_t* id; const uint16_t* sensor; const uint8_t* mask; const int32_t* labels;
  const int32_t* mesh_query;
  long long total;                                        // N * H * W, below 2^31
  int n_meshes, Q, bins, raw_lo, raw_hi;
  double unit, bin_m;
  unsigned int* hist;                                     // [Q][bins]
  unsigned long long* counts;                             // [Q][8]
  double* stats;                                          // [Q][4]
  int* range;                                             // workspace [Q][2]: the least and the greatest occupied bin
};

__global__ __launch_bounds__(DR_THREADS) void depth_init_kernel(const DepthParams p) {
  const long long i = (long long)blockIdx.x * DR_THREADS + threadIdx.x;
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

// the slot of query q in this workgroup, claiming a free one; -1 when all are taken by others
__device__ __forceinline__ int find_slot(DepthLds& s, int q) {
#pragma unroll
  for (int i = 0; i < DR_SLOTS; ++i) {
    int v = *(volatile int*)&s.query[i];
    if (v == 0) {
      const int old = atomicCAS(&s.query[i], 0, q + 1);
      v = old == 0 ? q + 1 : old;
    }
    if (v == q + 1) return i;
  }
  return -1;
}

// what the rule makes of one pixel: its query (-1: the pixel is skipped), the count it ends in (DR_OFF_MASK .. DR_IN_RANGE) and its bin
struct Pixel { int q, where, k; };

// one pixel by the rule of include/hamer_hip.h: e < total is its index, id its value of pred_id.  Nothing is added here.
__device__ __forceinline__ Pixel classify(const DepthParams& p, long long e, int id) {
  Pixel px = {-1, DR_OFF_MASK, 0};
  if (id < 0 || id >= p.n_meshes) return px;
  const int q = p.mesh_query[id];
  if (q < 0 || q >= p.Q) return px;
  px.q = q;
  const int label = (p.mask && p.labels) ? p.labels[q] : -2;
  if (label != -2) {
    const int m = (int)p.mask[e];
    if (!(label == -1 ? m != 0 : m == label)) return px;
  }
  const int raw = (int)p.sensor[e];
  px.where = DR_NO_MEASUREMENT;
  if (raw == 0 || raw < p.raw_lo || raw > p.raw_hi) return px;
  const double r = (double)raw * p.unit - (double)p.depth[e];
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

// Adds one pixel per lane.  The WHOLE wave calls this (lanes without a pixel pass q = -1).  Neighbouring pixels mostly belong
// to one query and often to one bin, where one atomic per lane would queue 64 deep on one LDS address: so the lanes of a query
// are counted with ballots and added by one lane, and the lanes that share the first two bins met are added together too; the
// other bins get one atomic per lane.
__device__ __forceinline__ void tally(const DepthParams& p, DepthLds& s, const Pixel px, int lane) {
  unsigned long long todo = __ballot(px.q >= 0);
  while (todo) {                                                          // wave-uniform: one turn per query among the 64 pixels
    const int leader = __ffsll((long long)todo) - 1;
    const int q = __shfl(px.q, leader);
    const bool mine = px.q == q;
    const unsigned long long group = __ballot(mine);
    todo &= ~group;
    int slot = -1, base = -1;
    const bool in_range = mine && px.where == DR_IN_RANGE;
    const unsigned long long placed = __ballot(in_range);
    const int k_first = placed ? __shfl(px.k, __ffsll((long long)placed) - 1) : 0;
    if (lane == leader) {
      slot = find_slot(s, q);
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
      add_count(p, s, slot, q, DR_COVERED, __popcll(group));
      add_count(p, s, slot, q, DR_IN_RANGE, __popcll(placed));
    }
    slot = __shfl(slot, leader);
    base = __shfl(base, leader);
#pragma unroll
    for (int which = DR_OFF_MASK; which <= DR_ABOVE; ++which) {
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
  }
}

__global__ __launch_bounds__(DR_THREADS) void depth_scan_kernel(const DepthParams p) {
  __shared__ DepthLds s;
  const int t = (int)threadIdx.x, lane = t & 63;
  for (int i = t; i < DR_SLOTS * DR_WINDOW; i += DR_THREADS) (&s.hist[0][0])[i] = 0u;
  if (t < DR_SLOTS * 8) (&s.cnt[0][0])[t] = 0u;
  if (t < DR_SLOTS) { s.query[t] = 0; s.base[t] = -1; s.lo[t] = 0x7fffffff; s.hi[t] = -1; }
  __syncthreads();

  long long head = (long long)((16u - (unsigned)((uintptr_t)p.id & 15u)) & 15u) >> 2;      // pixels before the first aligned address
  if (head > p.total) head = p.total;
  const long long nvec = (p.total - head) >> 2;
  const long long tail0 = head + (nvec << 2);                                                // first pixel behind the last whole vector
  const int4* __restrict__ vec = reinterpret_cast<const int4*>(p.id + head);
  const long long v0 = (long long)blockIdx.x * DR_VECS;
  for (int round = 0; round < DR_ROUNDS; ++round) {
    int4 v[DR_UNROLL];
    long long at[DR_UNROLL];
#pragma unroll
    for (int u = 0; u < DR_UNROLL; ++u) {
      at[u] = v0 + ((long long)round * DR_UNROLL + u) * DR_THREADS + t;
      v[u] = make_int4(-1, -1, -1, -1);
      if (at[u] < nvec) v[u] = vec[at[u]];                                                   // head + 4 at + 3 < tail0 <= total
    }
#pragma unroll
    for (int u = 0; u < DR_UNROLL; ++u) {
      const bool covered = (v[u].x & v[u].y & v[u].z & v[u].w) != -1;
      if (!__ballot(covered)) continue;                                                      // the wave's 256 pixels are uncovered
      const long long e = head + (at[u] << 2);                                               // (not used by a lane past nvec: its ids are -1)
      tally(p, s, classify(p, e, v[u].x), lane); tally(p, s, classify(p, e + 1, v[u].y), lane);
      tally(p, s, classify(p, e + 2, v[u].z), lane); tally(p, s, classify(p, e + 3, v[u].w), lane);
    }
  }
  if (blockIdx.x == 0 && t < 64) {
    // the scalar head (lanes 0..3) and tail (lanes 4..7) of the first wave
    long long e = -1;
    if (t < 4) e = t < head ? (long long)t : -1;
    else if (t < 8) e = tail0 + (t - 4) < p.total ? tail0 + (t - 4) : -1;
    tally(p, s, classify(p, e < 0 ? 0 : e, e < 0 ? -1 : p.id[e]), lane);
  }
  __syncthreads();

  // what the workgroup gathered goes to memory: one atomic per non-zero cell
  for (int i = t; i < DR_SLOTS * DR_WINDOW; i += DR_THREADS) {
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

bool positive_finite(double v) { return v > 0.0 && v < INFINITY; }

}  // namespace

extern "C" size_t hm_depth_residuals_workspace_bytes(int Q, int bins) {
  if (Q < 0 || bins < 2 || bins > DR_MAX_BINS || (bins & 1)) return 0;
  return (size_t)(Q < 1 ? 1 : Q) * 2 * sizeof(int);                        // never 0 for legal sizes: Q == 0 asks for one query's
}

extern "C" int hm_depth_residuals(const float* pred_depth, const int32_t* pred_id, const uint16_t* sensor, const uint8_t* mask,
                                  const int32_t* labels, int N, int H, int W, const int32_t* mesh_query, int n_meshes, int Q,
                                  double unit, int raw_lo, int raw_hi, double bin_m, int bins, uint32_t* hist, int64_t* counts,
                                  double* stats, void* workspace, size_t workspace_bytes, void* stream_) {
  if (N < 1 || H < 1 || W < 1) return hm_set_error(HM_ERR_ARG, "hm_depth_residuals: N, H and W must be positive");
  if ((long long)N * H * W >= (1ll << 31)) return hm_set_error(HM_ERR_ARG, "hm_depth_residuals: N * H * W must be below 2^31");
  if (Q < 0 || n_meshes < 0) return hm_set_error(HM_ERR_ARG, "hm_depth_residuals: Q and n_meshes must not be negative");
  if (bins < 2 || bins > DR_MAX_BINS || (bins & 1)) return hm_set_error(HM_ERR_ARG, "hm_depth_residuals: bins must be even and in 2..4096");
  if (!positive_finite(unit) || !positive_finite(bin_m)) return hm_set_error(HM_ERR_ARG, "hm_depth_residuals: unit and bin_m must be finite numbers > 0");
  if (raw_lo > raw_hi) return hm_set_error(HM_ERR_ARG, "hm_depth_residuals: raw_lo must not exceed raw_hi");
  if (!pred_depth || !pred_id || !sensor) return hm_set_error(HM_ERR_ARG, "hm_depth_residuals: null pred_depth, pred_id or sensor");
  if (Q == 0) return HM_OK;                                              // nothing to score: no launch, nothing else is read
  if ((n_meshes > 0 && !mesh_query) || !hist || !counts || !stats || !workspace)
    return hm_set_error(HM_ERR_ARG, "hm_depth_residuals: null mesh_query, hist, counts, stats or workspace");
  if (workspace_bytes < hm_depth_residuals_workspace_bytes(Q, bins))
    return hm_set_error(HM_ERR_ARG, "hm_depth_residuals: workspace too small (hm_depth_residuals_workspace_bytes)");
  if (((uintptr_t)counts & 7) || ((uintptr_t)stats & 7) || ((uintptr_t)hist & 3) || ((uintptr_t)workspace & 3))
    return hm_set_error(HM_ERR_ARG, "hm_depth_residuals: counts and stats must be 8-byte aligned, hist and workspace 4-byte");
  if (((uintptr_t)pred_depth & 3) || ((uintptr_t)pred_id & 3) || ((uintptr_t)sensor & 1) || ((uintptr_t)labels & 3) || ((uintptr_t)mesh_query & 3))
    return hm_set_error(HM_ERR_ARG, "hm_depth_residuals: pred_depth, pred_id, labels and mesh_query must be 4-byte aligned, sensor 2-byte");
  DepthParams p;
  p.depth = pred_depth; p.id = pred_id; p.sensor = sensor; p.mask = mask; p.labels = labels; p.mesh_query = mesh_query;
  p.total = (long long)N * H * W; p.n_meshes = n_meshes; p.Q = Q; p.bins = bins; p.raw_lo = raw_lo; p.raw_hi = raw_hi;
  p.unit = unit; p.bin_m = bin_m;
  p.hist = hist; p.counts = (unsigned long long*)counts; p.stats = stats; p.range = (int*)workspace;
  const long long cells = (long long)Q * bins > (long long)Q * 8 ? (long long)Q * bins : (long long)Q * 8;
  const long long init_blocks = (cells + DR_THREADS - 1) / DR_THREADS;
  if (init_blocks > 0x7fffffffll) return hm_set_error(HM_ERR_ARG, "hm_depth_residuals: Q * bins too large for one call");
  const long long vecs = p.total >> 2;                                   // an upper bound of the whole vectors
  const long long scan_blocks = vecs > 0 ? (vecs + DR_VECS - 1) / DR_VECS : 1;
  hipStream_t s = (hipStream_t)stream_;
  HmProfScope prof(HM_K_OTHER, 8, Q, H, W, s);
  hipLaunchKernelGGL(depth_init_kernel, dim3((unsigned)init_blocks), dim3(DR_THREADS), 0, s, p);
  int rc = hm_check_launch("hm_depth_residuals (init)");
  if (rc != HM_OK) return rc;
  hipLaunchKernelGGL(depth_scan_kernel, dim3((unsigned)scan_blocks), dim3(DR_THREADS), 0, s, p);
  rc = hm_check_launch("hm_depth_residuals (scan)");
  if (rc != HM_OK) return rc;
  hipLaunchKernelGGL(depth_stats_kernel, dim3((unsigned)Q), dim3(64), 0, s, p);
  return hm_check_launch("hm_depth_residuals (stats)");
}
