// hm_depth_fit - the rigid motion that brings the predicted hands' z-buffer onto a sensor depth map: per query the 6 x 6 normal
// equations of a point-to-plane fit over the pixels its meshes cover, seven pixel counts, and their damped Cholesky solution
// (include/hamer_hip.h, "Depth fit").
//
// The whole file is compiled without contraction (the pragma below) and every fp64 expression is written in the rule's order.
// Every pixel's 28 terms are rounded to integers (llrint of a correctly rounded quotient times 2^30) before they are added, so
// a query's sums and counts depend on nothing but its own pixels and the scalars -- not on Q, N, the order of the meshes or the
// grid; solution is a function of those integers and the scalars alone.
//
// Three kernels on the stream, no host synchronisation, no allocation:
//   init   zeroes the workspace: per query one row of 36 int64, the 28 sums followed by the 8 counts.
//   scan   ONE pass over the N * H * W pixels for all queries on depth_scan.h's walk, gate, query slots and groups of a wave
//          (shared with depth_eval.hip); the four neighbours, the camera and the pivot are read only for pixels whose residual is
//          within gate_m.  Within a group the counts are popcounts, and each of the 28 terms is added across the wave with 64-bit
//          shuffles (lanes outside the group add 0; integer adds commute, so the tree is exact) and then ONCE, by the group's
//          first lane, to the query's row in LDS with a 64-bit LDS add.  A workgroup keeps DF_SLOTS queries; a group whose query
//          found no slot adds its 28 wave totals straight to the workspace instead -- the same integers.  At the end the workgroup
//          adds its non-zero LDS cells to the workspace, one 64-bit atomic each, 36 consecutive cells per slot.
//   solve  one thread per query: copies its row to sums and counts, builds M, factorises and solves in the header's order.
#include <float.h>
#include <math.h>
#include "common.h"
#include "depth_scan.h"

#pragma clang fp contract(off)

namespace {
using namespace depth_scan;

constexpr int DF_SLOTS = 4, DF_SUMS = 28, DF_CELLS = 36;
constexpr double DF_SCALE = 1073741824.0, DF_INV_SCALE = 1.0 / 1073741824.0;     // 2^30 and 2^-30: exact
enum { DF_GATED = MEASURED, DF_NO_NORMAL = 4, DF_REJECTED = 5, DF_USED = 6 };     // the counts behind COVERED, OFF_MASK and NO_MEASUREMENT

struct FitParams : Maps {
  const double* cameras; const double* pivot;             // [N][4]: fx, fy, cx, cy, and [Q][3]
  unsigned int HW; int H, W, min_pixels;                  // HW = H * W
  double gate_m, edge_m, reach2, damping, lever2;         // reach2 = reach_m * reach_m, lever2 = lever_m * lever_m
  unsigned long long* acc;                                // workspace [Q][36]
  long long* sums;                                        // [Q][28]
  long long* counts;                                      // [Q][8]
  double* solution;                                       // [Q][8]
};

__global__ __launch_bounds__(THREADS) void fit_init_kernel(const FitParams p) {
  const long long i = (long long)blockIdx.x * THREADS + threadIdx.x;
  if (i < (long long)p.Q * DF_CELLS) p.acc[i] = 0ull;
}

struct FitLds {
  unsigned long long acc[DF_SLOTS][DF_CELLS];
  int query[DF_SLOTS];                                    // q + 1 of the slot's query, 0 while it is free
};

// what the rule makes of one pixel: its query (-1: the pixel is skipped), the count it ends in (OFF_MASK .. DF_USED) and,
// for a used pixel, J, rho and l2
struct FitPixel { int q, where; double J[6], rho, l2; };

// one pixel by the rule of include/hamer_hip.h: e < total is its index, id its value of pred_id.  Nothing is added here.
__device__ __forceinline__ FitPixel classify(const FitParams& p, unsigned int e, int id) {
  const Gate g = gate(p, e, id);
  FitPixel px;
  px.q = g.q; px.where = g.stage; px.rho = 0.0; px.l2 = 1.0;
#pragma unroll
  for (int i = 0; i < 6; ++i) px.J[i] = 0.0;
  if (g.q < 0 || g.stage != MEASURED) return px;
  const double d = (double)p.depth[e];
  const double rz = (double)g.raw * p.unit - d;
  if (!(fabs(rz) <= p.gate_m)) return px;                                     // DF_GATED; a NaN is gated
  px.where = DF_NO_NORMAL;
  const unsigned int n = e / p.HW, rem = e - n * p.HW;
  const int v = (int)(rem / (unsigned int)p.W), u = (int)(rem - (unsigned int)v * (unsigned int)p.W);
  if (u < 1 || u + 1 >= p.W || v < 1 || v + 1 >= p.H) return px;              // so e - W >= 0 and e + W < total below
  if (p.id[e - 1] != id || p.id[e + 1] != id || p.id[e - p.W] != id || p.id[e + p.W] != id) return px;
  const double dl = (double)p.depth[e - 1], dr = (double)p.depth[e + 1], du = (double)p.depth[e - p.W], dd = (double)p.depth[e + p.W];
  if (!(fabs(dl - d) <= p.edge_m) || !(fabs(dr - d) <= p.edge_m) || !(fabs(du - d) <= p.edge_m) || !(fabs(dd - d) <= p.edge_m)) return px;
  const double* cam = p.cameras + (size_t)n * 4;
  const double fx = cam[0], fy = cam[1], cx = cam[2], cy = cam[3];
  const double rx = ((double)u - cx) / fx, rxl = ((double)(u - 1) - cx) / fx, rxr = ((double)(u + 1) - cx) / fx;
  const double ry = ((double)v - cy) / fy, ryu = ((double)(v - 1) - cy) / fy, ryd = ((double)(v + 1) - cy) / fy;
  const double ax = dr * rxr - dl * rxl, ay = dr * ry - dl * ry, az = dr - dl;
  const double bx = dd * rx - du * rx, by = dd * ryd - du * ryu, bz = dd - du;
  const double nx = ay * bz - az * by, ny = az * bx - ax * bz, nz = ax * by - ay * bx;
  const double l2 = nx * nx + ny * ny + nz * nz;
  const double* pv = p.pivot + (size_t)g.q * 3;
  const double mx = d * rx - pv[0], my = d * ry - pv[1], mz = d - pv[2];
  const double rho = (nx * rx + ny * ry + nz) * rz;
  const double mm = mx * mx + my * my + mz * mz;
  px.where = DF_REJECTED;
  if (!(l2 > 0.0 && l2 <= DBL_MAX) || mm > p.reach2 || rho * rho > l2) return px;
  px.where = DF_USED;
  px.J[0] = my * nz - mz * ny; px.J[1] = mz * nx - mx * nz; px.J[2] = mx * ny - my * nx;
  px.J[3] = nx; px.J[4] = ny; px.J[5] = nz;
  px.rho = rho; px.l2 = l2;
  return px;
}

__device__ __forceinline__ void add_cell(const FitParams& p, FitLds& s, int slot, int q, int cell, long long n) {
  if (n == 0) return;
  // workgroup scope: all an LDS cell needs, and it keeps hipcc from merging both adds into ONE flat atomic on a selected address
  // (whenever tally or for_each_query changes, count flat_atomic in fit_scan_kernel's ISA again: 0, with 70 ds_add_u64)
  if (slot >= 0) __hip_atomic_fetch_add(&s.acc[slot][cell], (unsigned long long)n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  else atomicAdd(p.acc + (size_t)q * DF_CELLS + cell, (unsigned long long)n);
}

__device__ __forceinline__ long long wave_sum(long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// Adds one pixel per lane; the WHOLE wave calls this (depth_scan.h, for_each_query).
__device__ __forceinline__ void tally(const FitParams& p, FitLds& s, const FitPixel& px, int lane) {
  for_each_query(px.q, [&](int leader, int q, bool mine, unsigned long long group) {
    int slot = -1;
    if (lane == leader) slot = find_slot(s.query, q);
    slot = __shfl(slot, leader);
    if (lane == leader) add_cell(p, s, slot, q, DF_SUMS + COVERED, __popcll(group));
#pragma unroll
    for (int which = OFF_MASK; which <= DF_USED; ++which) {
      const int n = __popcll(__ballot(mine && px.where == which));
      if (lane == leader) add_cell(p, s, slot, q, DF_SUMS + which, n);
    }
    const bool use = mine && px.where == DF_USED;
    if (!__ballot(use)) return;
    int cell = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
#pragma unroll
      for (int j = i; j < 6; ++j) {
        const long long t = wave_sum(use ? llrint((px.J[i] * px.J[j]) / px.l2 * DF_SCALE) : 0ll);
        if (lane == leader) add_cell(p, s, slot, q, cell, t);
        ++cell;
      }
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      const long long t = wave_sum(use ? llrint((px.J[i] * px.rho) / px.l2 * DF_SCALE) : 0ll);
      if (lane == leader) add_cell(p, s, slot, q, 21 + i, t);
    }
    const long long t = wave_sum(use ? llrint((px.rho * px.rho) / px.l2 * DF_SCALE) : 0ll);
    if (lane == leader) add_cell(p, s, slot, q, 27, t);
  });
}

__global__ __launch_bounds__(THREADS) void fit_scan_kernel(const FitParams p) {
  __shared__ FitLds s;
  const int t = (int)threadIdx.x, lane = t & 63;
  if (t < DF_SLOTS * DF_CELLS) (&s.acc[0][0])[t] = 0ull;
  if (t < DF_SLOTS) s.query[t] = 0;
  __syncthreads();

  const Walk w = walk_of(p.id, p.total);
  for (int round = 0; round < ROUNDS; ++round) {
    int4 v[UNROLL];
    const long long e0 = load_round(w, round, t, v);
    unsigned int live = 0;
#pragma unroll
    for (int u = 0; u < UNROLL; ++u)
      if (__ballot((v[u].x & v[u].y & v[u].z & v[u].w) != -1)) live |= 1u << u;              // wave-uniform
    if (!live) continue;                                                                     // the wave's 1024 pixels are uncovered
    // one copy of the per-pixel code for the 16 pixels of a lane: the vectors and their components are shifted through
    // `cur` with moves, so that nothing is indexed by k
    int4 cur = v[0];
#pragma clang loop unroll(disable)
    for (int k = 0; k < 4 * UNROLL; ++k) {
      const int u = k >> 2, c = k & 3;
      if (c == 0 && k != 0) { cur = v[1]; v[1] = v[2]; v[2] = v[3]; }
      const int id = cur.x;
      cur.x = cur.y; cur.y = cur.z; cur.z = cur.w;
      if (!((live >> u) & 1u)) continue;
      if (!__ballot(id >= 0)) continue;
      const FitPixel px = classify(p, (unsigned int)(e0 + (long long)u * (4 * THREADS) + c), id);
      tally(p, s, px, lane);
    }
  }
  scan_edges(w, p.id, t, [&](long long e, int id) { tally(p, s, classify(p, (unsigned int)e, id), lane); });
  __syncthreads();

  // what the workgroup gathered goes to memory: one atomic per non-zero cell, a slot's 36 cells side by side
  if (t < DF_SLOTS * DF_CELLS) {
    const unsigned long long n = (&s.acc[0][0])[t];
    const int slot = t / DF_CELLS;
    if (n != 0ull) atomicAdd(p.acc + (size_t)(s.query[slot] - 1) * DF_CELLS + (t - slot * DF_CELLS), n);
  }
}

__global__ __launch_bounds__(64) void fit_solve_kernel(const FitParams p) {
  const int q = (int)blockIdx.x * 64 + (int)threadIdx.x;
  if (q >= p.Q) return;
  const unsigned long long* row = p.acc + (size_t)q * DF_CELLS;
  long long sum[DF_SUMS];
#pragma unroll
  for (int i = 0; i < DF_SUMS; ++i) { sum[i] = (long long)row[i]; p.sums[(size_t)q * DF_SUMS + i] = sum[i]; }
#pragma unroll
  for (int i = 0; i < 7; ++i) p.counts[(size_t)q * 8 + i] = (long long)row[DF_SUMS + i];
  p.counts[(size_t)q * 8 + 7] = 0;
  const long long used = (long long)row[DF_SUMS + DF_USED];
  const double nan = __longlong_as_double(0x7ff8000000000000ll);

  double M[6][6], g[6];
  {
    int k = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
#pragma unroll
      for (int j = i; j < 6; ++j) { M[i][j] = (double)sum[k] * DF_INV_SCALE; M[j][i] = M[i][j]; ++k; }
    }
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) g[i] = (double)sum[21 + i] * DF_INV_SCALE;
  const double du = p.damping * (double)used;
#pragma unroll
  for (int i = 0; i < 3; ++i) M[i][i] = M[i][i] + du * p.lever2;
#pragma unroll
  for (int i = 3; i < 6; ++i) M[i][i] = M[i][i] + du;

  // Cholesky M = L L^T, column by column, every inner sum from k = 0 upwards
  double Lm[6][6];
  bool ok = used >= (long long)p.min_pixels;
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    double sj = M[j][j];
#pragma unroll
    for (int k = 0; k < j; ++k) sj = sj - Lm[j][k] * Lm[j][k];
    if (!(sj > 0.0)) ok = false;
    Lm[j][j] = sqrt(sj);
#pragma unroll
    for (int i = j + 1; i < 6; ++i) {
      double sij = M[i][j];
#pragma unroll
      for (int k = 0; k < j; ++k) sij = sij - Lm[i][k] * Lm[j][k];
      Lm[i][j] = sij / Lm[j][j];
    }
  }
  double y[6], x[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    double si = g[i];
#pragma unroll
    for (int k = 0; k < i; ++k) si = si - Lm[i][k] * y[k];
    y[i] = si / Lm[i][i];
  }
#pragma unroll
  for (int i = 5; i >= 0; --i) {
    double si = y[i];
#pragma unroll
    for (int k = i + 1; k < 6; ++k) si = si - Lm[k][i] * x[k];
    x[i] = si / Lm[i][i];
  }
  double* out = p.solution + (size_t)q * 8;
#pragma unroll
  for (int i = 0; i < 6; ++i) out[i] = ok ? x[i] : 0.0;
  out[6] = used > 0 ? sqrt(((double)sum[27] * DF_INV_SCALE) / (double)used) : nan;
  out[7] = ok ? 1.0 : 0.0;
}

}  // namespace

extern "C" size_t hm_depth_fit_workspace_bytes(int Q) {
  if (Q < 0) return 0;
  return (size_t)(Q < 1 ? 1 : Q) * DF_CELLS * sizeof(unsigned long long);  // never 0 for a legal Q: Q == 0 asks for one query's
}

extern "C" int hm_depth_fit(const float* pred_depth, const int32_t* pred_id, const uint16_t* sensor, const uint8_t* mask,
                            const int32_t* labels, int N, int H, int W, const int32_t* mesh_query, int n_meshes, int Q,
                            const double* cameras, const double* pivot, double unit, int raw_lo, int raw_hi, double gate_m,
                            double edge_m, double reach_m, double damping, double lever_m, int min_pixels, int64_t* sums,
                            int64_t* counts, double* solution, void* workspace, size_t workspace_bytes, void* stream_) {
  FitParams p;
  p.depth = pred_depth; p.id = pred_id; p.sensor = sensor; p.mask = mask; p.labels = labels; p.mesh_query = mesh_query;
  p.cameras = cameras; p.pivot = pivot;
  p.HW = (unsigned int)((long long)H * W); p.H = H; p.W = W;
  p.n_meshes = n_meshes; p.Q = Q; p.raw_lo = raw_lo; p.raw_hi = raw_hi; p.min_pixels = min_pixels;
  p.unit = unit; p.gate_m = gate_m; p.edge_m = edge_m; p.reach2 = reach_m * reach_m; p.damping = damping; p.lever2 = lever_m * lever_m;
  p.acc = (unsigned long long*)workspace; p.sums = (long long*)sums; p.counts = (long long*)counts; p.solution = solution;
  const char* unit_text = !positive_finite(unit) ? "unit must be a finite number > 0" : nullptr;
  const char* scalars = !(gate_m > 0.0 && gate_m <= 0.25)   ? "gate_m must be in (0, 0.25]"
      : !positive_finite(edge_m)                            ? "edge_m must be a finite number > 0"
      : !(reach_m > 0.0 && reach_m <= 1.0)                  ? "reach_m must be in (0, 1]"
      : !(damping >= 0.0 && damping < INFINITY)             ? "damping must be a finite number >= 0"
      : !positive_finite(lever_m)                           ? "lever_m must be a finite number > 0"
      : min_pixels < 1                                      ? "min_pixels must be at least 1" : nullptr;
  const char* buffers = ((n_meshes > 0 && !mesh_query) || !cameras || !pivot || !sums || !counts || !solution || !workspace)
          ? "null mesh_query, cameras, pivot, sums, counts, solution or workspace"
      : workspace_bytes < hm_depth_fit_workspace_bytes(Q) ? "workspace too small (hm_depth_fit_workspace_bytes)"
      : (((uintptr_t)sums & 7) || ((uintptr_t)counts & 7) || ((uintptr_t)solution & 7) || ((uintptr_t)workspace & 7) ||
         ((uintptr_t)cameras & 7) || ((uintptr_t)pivot & 7))
          ? "sums, counts, solution, workspace, cameras and pivot must be 8-byte aligned" : nullptr;
  int rc = host_checks("hm_depth_fit", p, N, H, W, unit_text, scalars, buffers);
  if (rc != HM_OK || Q == 0) return rc;                                  // no query, nothing to fit: no launch
  const long long init_blocks = ((long long)Q * DF_CELLS + THREADS - 1) / THREADS;
  hipStream_t s = (hipStream_t)stream_;
  HmProfScope prof(HM_K_OTHER, 9, Q, H, W, s);
  hipLaunchKernelGGL(fit_init_kernel, dim3((unsigned)init_blocks), dim3(THREADS), 0, s, p);
  rc = hm_check_launch("hm_depth_fit (init)");
  if (rc != HM_OK) return rc;
  hipLaunchKernelGGL(fit_scan_kernel, dim3(scan_blocks(p.total)), dim3(THREADS), 0, s, p);
  rc = hm_check_launch("hm_depth_fit (scan)");
  if (rc != HM_OK) return rc;
  hipLaunchKernelGGL(fit_solve_kernel, dim3((unsigned)((Q + 63) / 64)), dim3(64), 0, s, p);
  return hm_check_launch("hm_depth_fit (solve)");
}
