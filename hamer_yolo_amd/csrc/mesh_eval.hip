// hm_mesh_score, hm_pck_auc - the two halves of the hand-mesh tables that hm_pose_eval does not produce: the F-score of two
// point clouds at distance thresholds (F@5 mm, F@15 mm of FreiHAND / HO3D) and the area under the PCK curve (get_measures,
// _get_pck of rootnet/KeypointFusion/util/eval_utils.py, for any number of keypoints).
//
// Every fp64 operation in this file is a plain IEEE operation in the order written: no FMA contraction (the pragma below), no
// fast-math.  The tests compare counts exactly, distances to one fp32 rounding and the PCK curve bit for bit on that ground.
//
// The score.  One 1024-thread workgroup owns one hand.  The participating points of both sets are staged once in LDS as fp64,
// after the root subtraction and (pred only) the similarity transform of hm_pose_eval: 2 x 1024 x 3 x 8 = 48 KiB.  Thread t owns
// pred point t (a point per thread: sixteen waves hide the fp64 latency) and scans every gt point from LDS (all lanes read one address: a broadcast); then the roles
// swap.  d^2 = (dx dx + dy dy) + dz dz; the running minimum takes a NaN candidate and keeps it (numpy.min); one sqrt follows.
// The threshold counts are integers, summed by LDS atomics: no order question.  Nothing of a hand depends on another hand.
//
// The PCK curve.  The thresholds are np.linspace(val_min, val_max, steps): i * step + start with step = (stop - start) / (steps - 1)
// and the last one set to stop; they never decrease, so #(err <= thr[i]) is a prefix sum of the histogram over "the first i
// with err <= thr[i]" (binary search with that very comparison; a NaN finds none and is a miss).  A workgroup owns 32
// keypoints x one chunk of samples: lanes run along K (coalesced rows), the histogram is built in LDS with integer atomics and
// flushed with 64-bit integer atomics into the workspace, which the call zeroes on the stream first.  Integer sums: the result
// does not depend on the chunking.  One finishing workgroup turns counts into pck = count / N (one division: the bits of
// numpy's mean of 0 / 1), the trapezoid areas, their mean and the mean curve (summed over keypoints in ascending order, as
// numpy reduces axis 0).
#include <math.h>
#include <stdio.h>
#include "common.h"
#include "hamer_hip_internal.h"

#pragma clang fp contract(off)

namespace {

constexpr int MS_MAX_POINTS = 1024, MS_MAX_THR = 8, MS_THREADS = 1024;
constexpr int PCK_MAX_STEPS = 256, PCK_KT = 32, PCK_ROWS = 8, PCK_PITCH = PCK_MAX_STEPS + 1, PCK_DEFAULT_CHUNK = 256;
constexpr int PCK_MAX_CHUNKS = 65535, PCK_FINISH_THREADS = 1024;

struct MeshScoreParams {
  const float* pred; const float* gt; const float* transform;
  int P, Q, gt_stride, root, p_lo, n_p, g_lo, n_g, n_thr;
  double thr[MS_MAX_THR];
  float* d_pred; float* d_gt; float* precision; float* recall; float* fscore; float* point_err;
};

// the nearest of the n points at `other` (LDS, [n][3] fp64) to a: its squared distance, NaN if any candidate's is
__device__ __forceinline__ double nearest_d2(const double* a, const double* other, int n) {
  double m = INFINITY;
  for (int j = 0; j < n; ++j) {
    const double dx = a[0] - other[j * 3 + 0], dy = a[1] - other[j * 3 + 1], dz = a[2] - other[j * 3 + 2];
    const double d2 = (dx * dx + dy * dy) + dz * dz;
    m = (d2 < m || d2 != d2) ? d2 : m;                                  // a NaN enters and then stays (d2 < NaN is false)
  }
  return m;
}

__global__ __launch_bounds__(MS_THREADS) void mesh_score_kernel(const MeshScoreParams p) {
  __shared__ double sp[MS_MAX_POINTS * 3], sg[MS_MAX_POINTS * 3];
  __shared__ int cnt[2][MS_MAX_THR];
  const int hand = blockIdx.x, tid = threadIdx.x;
  const float* __restrict__ pr = p.pred + (size_t)hand * p.P * 3;
  const float* __restrict__ gr = p.gt + (size_t)hand * p.Q * p.gt_stride;
  double r1[3] = {0.0, 0.0, 0.0}, r2[3] = {0.0, 0.0, 0.0};
  if (p.root >= 0) {
#pragma unroll
    for (int k = 0; k < 3; ++k) { r1[k] = (double)pr[(size_t)p.root * 3 + k]; r2[k] = (double)gr[(size_t)p.root * p.gt_stride + k]; }
  }
  double scale = 1.0, R[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}}, t[3] = {0.0, 0.0, 0.0};
  if (p.transform) {
    const float* __restrict__ tr = p.transform + (size_t)hand * 13;
    scale = (double)tr[0];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
      for (int j = 0; j < 3; ++j) R[i][j] = (double)tr[1 + i * 3 + j];
      t[i] = (double)tr[10 + i];
    }
  }
  if (tid < 2 * MS_MAX_THR) (&cnt[0][0])[tid] = 0;

  // ---- the only read of the inputs: root subtracted, pred transformed, both kept in fp64
  for (int i = tid; i < p.n_p; i += MS_THREADS) {
    double a[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) a[k] = (double)pr[(size_t)(p.p_lo + i) * 3 + k] - r1[k];
#pragma unroll
    for (int k = 0; k < 3; ++k)
      sp[i * 3 + k] = p.transform ? scale * (R[k][0] * a[0] + R[k][1] * a[1] + R[k][2] * a[2]) + t[k] : a[k];
  }
  for (int i = tid; i < p.n_g; i += MS_THREADS) {
#pragma unroll
    for (int k = 0; k < 3; ++k) sg[i * 3 + k] = (double)gr[(size_t)(p.g_lo + i) * p.gt_stride + k] - r2[k];
  }
  __syncthreads();

  // ---- pred -> gt, then gt -> pred
#pragma unroll
  for (int side = 0; side < 2; ++side) {
    const double* mine = side == 0 ? sp : sg;
    const double* other = side == 0 ? sg : sp;
    const int n_mine = side == 0 ? p.n_p : p.n_g, n_other = side == 0 ? p.n_g : p.n_p;
    float* __restrict__ out = side == 0 ? p.d_pred : p.d_gt;
    const bool counts = side == 0 ? (p.precision || p.fscore) : (p.recall || p.fscore);
    if (!out && !counts) continue;
    int c[MS_MAX_THR];
#pragma unroll
    for (int j = 0; j < MS_MAX_THR; ++j) c[j] = 0;
    for (int i = tid; i < n_mine; i += MS_THREADS) {
      const double a[3] = {mine[i * 3 + 0], mine[i * 3 + 1], mine[i * 3 + 2]};
      const double d = sqrt(nearest_d2(a, other, n_other));
      if (out) out[(size_t)hand * n_mine + i] = (float)d;
#pragma unroll
      for (int j = 0; j < MS_MAX_THR; ++j) c[j] += (j < p.n_thr && d < p.thr[j]) ? 1 : 0;      // strict; NaN is no hit
    }
    if (counts) {
#pragma unroll
      for (int j = 0; j < MS_MAX_THR; ++j)
        if (c[j]) atomicAdd(&cnt[side][j], c[j]);
    }
  }

  // ---- corresponding points (n_p == n_g: the host has checked)
  if (p.point_err) {
    for (int i = tid; i < p.n_p; i += MS_THREADS) {
      const double dx = sp[i * 3 + 0] - sg[i * 3 + 0], dy = sp[i * 3 + 1] - sg[i * 3 + 1], dz = sp[i * 3 + 2] - sg[i * 3 + 2];
      p.point_err[(size_t)hand * p.n_p + i] = (float)sqrt((dx * dx + dy * dy) + dz * dz);
    }
  }
  __syncthreads();
  if (tid < p.n_thr) {
    const double pv = (double)cnt[0][tid] / (double)p.n_p, rv = (double)cnt[1][tid] / (double)p.n_g;
    const size_t o = (size_t)hand * p.n_thr + tid;
    if (p.precision) p.precision[o] = (float)pv;
    if (p.recall) p.recall[o] = (float)rv;
    if (p.fscore) p.fscore[o] = (float)(pv + rv == 0.0 ? 0.0 : 2.0 * pv * rv / (pv + rv));
  }
}

// ------------------------------------------------------------------ PCK curve and its area
struct PckParams {
  const float* err; long long N; int K; long long ld; double start, stop, step; int T; long long chunk;
  unsigned long long* counts;                                           // [T][K], zeroed by the call
  double* pck; double* auc; double* mean_auc; double* curve; double* thr_out;
};

__device__ __forceinline__ double pck_threshold(const PckParams& p, int i) {
  return i == p.T - 1 ? p.stop : (double)i * p.step + p.start;         // np.linspace: arange * step + start, y[-1] = stop
}

__global__ __launch_bounds__(PCK_KT * PCK_ROWS) void pck_hist_kernel(const PckParams p) {
  __shared__ double thr[PCK_MAX_STEPS];
  __shared__ unsigned hist[PCK_KT * PCK_PITCH];
  const int tid = threadIdx.x, kk = tid & (PCK_KT - 1), row = tid / PCK_KT;
  for (int i = tid; i < PCK_KT * PCK_PITCH; i += PCK_KT * PCK_ROWS) hist[i] = 0u;
  if (tid < p.T) thr[tid] = pck_threshold(p, tid);
  __syncthreads();
  const int k0 = blockIdx.x * PCK_KT, k = k0 + kk;
  const long long n0 = (long long)blockIdx.y * p.chunk;
  const long long n1 = n0 + p.chunk < p.N ? n0 + p.chunk : p.N;
  if (k < p.K) {
    for (long long n = n0 + row; n < n1; n += PCK_ROWS) {
      const double e = (double)p.err[(size_t)n * (size_t)p.ld + k];
      int lo = 0, hi = p.T;                                             // the first i with e <= thr[i]; T when there is none (NaN too)
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (e <= thr[mid]) hi = mid; else lo = mid + 1;
      }
      if (lo < p.T) atomicAdd(&hist[kk * PCK_PITCH + lo], 1u);
    }
  }
  __syncthreads();
  for (int i = tid; i < PCK_KT * p.T; i += PCK_KT * PCK_ROWS) {                      // counts is [T][K]: lanes along K here too
    const int b = i / PCK_KT, k2 = i & (PCK_KT - 1);
    const unsigned v = hist[k2 * PCK_PITCH + b];
    if (v && k0 + k2 < p.K) atomicAdd(&p.counts[(size_t)b * p.K + (k0 + k2)], (unsigned long long)v);
  }
}

// v[0] + v[stride] + ... (n terms), added strictly in that order
__device__ __forceinline__ double ordered_sum(const double* v, size_t stride, int n) {
  double s = 0.0;
  int k = 0;
  for (; k + 32 <= n; k += 32) {
    double x[32];
#pragma unroll
    for (int j = 0; j < 32; ++j) x[j] = v[(size_t)(k + j) * stride];
#pragma unroll
    for (int j = 0; j < 32; ++j) s += x[j];
  }
  for (; k < n; ++k) s += v[(size_t)k * stride];
  return s;
}

__global__ __launch_bounds__(PCK_FINISH_THREADS) void pck_finish_kernel(const PckParams p) {
  __shared__ double thr[PCK_MAX_STEPS];
  __shared__ double norm;
  const int tid = threadIdx.x;
  if (tid < p.T) {
    thr[tid] = pck_threshold(p, tid);
    if (p.thr_out) p.thr_out[tid] = thr[tid];
  }
  __syncthreads();
  if (tid == 0) {
    double s = 0.0;
    for (int i = 0; i + 1 < p.T; ++i) s += (thr[i + 1] - thr[i]) * (1.0 + 1.0) / 2.0;
    norm = s;
  }
  __syncthreads();
  const unsigned long long* __restrict__ counts = p.counts;             // read only here: its loads may pass the stores below
  for (int k = tid; k < p.K; k += PCK_FINISH_THREADS) {
    unsigned long long run = 0ull;
    double prev = 0.0, area = 0.0;
#pragma unroll 4
    for (int i = 0; i < p.T; ++i) {
      run += counts[(size_t)i * p.K + k];
      const double y = (double)run / (double)p.N;
      p.pck[(size_t)k * p.T + i] = y;
      if (i > 0) area += (thr[i] - thr[i - 1]) * (y + prev) / 2.0;
      prev = y;
    }
    p.auc[k] = area / norm;
  }
  __syncthreads();                                                      // pck and auc of this workgroup's own stores
  // both means add in ascending k, one after the other (numpy's order over axis 0); the loads go out 32 at a time
  if (p.curve && tid < p.T) p.curve[tid] = ordered_sum(p.pck + tid, p.T, p.K) / (double)p.K;
  if (p.mean_auc && tid == PCK_FINISH_THREADS - 1) *p.mean_auc = ordered_sum(p.auc, 1, p.K) / (double)p.K;
}

long long pck_chunk_rows(long long N, long long asked) {
  long long chunk = asked > 0 ? asked : PCK_DEFAULT_CHUNK;
  const long long least = (N + PCK_MAX_CHUNKS - 1) / PCK_MAX_CHUNKS;   // the grid's y extent is 65535 at the most
  return chunk < least ? least : chunk;
}

}  // namespace

extern "C" int hm_mesh_score(const hm_mesh_score_args* a, void* stream_) {
  if (!a) return hm_set_error(HM_ERR_ARG, "hm_mesh_score: null args");
  if (!a->pred || !a->gt) return hm_set_error(HM_ERR_ARG, "hm_mesh_score: null pred or gt");
  if (a->B <= 0) return hm_set_error(HM_ERR_ARG, "hm_mesh_score: B must be positive");
  if (a->P < 1 || a->P > MS_MAX_POINTS) return hm_set_error(HM_ERR_ARG, "hm_mesh_score: P must be in 1..1024");
  if (a->Q < 1 || a->Q > MS_MAX_POINTS) return hm_set_error(HM_ERR_ARG, "hm_mesh_score: Q must be in 1..1024");
  if (a->gt_stride != 3 && a->gt_stride != 4) return hm_set_error(HM_ERR_ARG, "hm_mesh_score: gt_stride must be 3 or 4");
  if (a->root < -1 || a->root >= a->P || a->root >= a->Q)
    return hm_set_error(HM_ERR_ARG, "hm_mesh_score: root must be -1 or an index into both sets");
  if (a->pred_lo < 0 || a->pred_n < 1 || a->pred_n > a->P - a->pred_lo)
    return hm_set_error(HM_ERR_ARG, "hm_mesh_score: pred range must lie inside 0..P with at least one point");
  if (a->gt_lo < 0 || a->gt_n < 1 || a->gt_n > a->Q - a->gt_lo)
    return hm_set_error(HM_ERR_ARG, "hm_mesh_score: gt range must lie inside 0..Q with at least one point");
  if (a->n_thr < 0 || a->n_thr > MS_MAX_THR) return hm_set_error(HM_ERR_ARG, "hm_mesh_score: at most 8 thresholds");
  if ((a->precision || a->recall || a->fscore) && a->n_thr == 0)
    return hm_set_error(HM_ERR_ARG, "hm_mesh_score: precision, recall and fscore need at least one of the thresholds");
  if (a->point_err && a->pred_n != a->gt_n)
    return hm_set_error(HM_ERR_ARG, "hm_mesh_score: point_err needs equal participating counts");
  if (!a->d_pred && !a->d_gt && !a->precision && !a->recall && !a->fscore && !a->point_err)
    return hm_set_error(HM_ERR_ARG, "hm_mesh_score: no output requested");
  if (((uintptr_t)a->pred & 3) || ((uintptr_t)a->gt & 3) || ((uintptr_t)a->transform & 3))
    return hm_set_error(HM_ERR_ARG, "hm_mesh_score: pred, gt and transform must be 4-byte aligned");
  MeshScoreParams p;
  p.pred = a->pred; p.gt = a->gt; p.transform = a->transform;
  p.P = a->P; p.Q = a->Q; p.gt_stride = a->gt_stride; p.root = a->root;
  p.p_lo = a->pred_lo; p.n_p = a->pred_n; p.g_lo = a->gt_lo; p.n_g = a->gt_n; p.n_thr = a->n_thr;
  for (int j = 0; j < MS_MAX_THR; ++j) p.thr[j] = j < a->n_thr ? a->thresholds[j] : 0.0;
  p.d_pred = a->d_pred; p.d_gt = a->d_gt; p.precision = a->precision; p.recall = a->recall; p.fscore = a->fscore;
  p.point_err = a->point_err;
  HmProfScope prof(HM_K_OTHER, 0, a->B, a->pred_n, a->gt_n, (hipStream_t)stream_);
  hipLaunchKernelGGL(mesh_score_kernel, dim3((unsigned)a->B), dim3(MS_THREADS), 0, (hipStream_t)stream_, p);
  return hm_check_launch("hm_mesh_score");
}

extern "C" size_t hm_pck_auc_workspace_bytes(int K, int steps) {
  if (K < 1 || steps < 2 || steps > PCK_MAX_STEPS) return 0;
  return (size_t)K * (size_t)steps * sizeof(unsigned long long);
}

extern "C" int hm_pck_auc(const hm_pck_auc_args* a, void* stream_) {
  if (!a) return hm_set_error(HM_ERR_ARG, "hm_pck_auc: null args");
  if (!a->err || !a->pck || !a->auc) return hm_set_error(HM_ERR_ARG, "hm_pck_auc: null err, pck or auc");
  if (a->N <= 0) return hm_set_error(HM_ERR_ARG, "hm_pck_auc: N must be positive");
  if (a->K < 1) return hm_set_error(HM_ERR_ARG, "hm_pck_auc: K must be positive");
  if (a->ld < a->K) return hm_set_error(HM_ERR_ARG, "hm_pck_auc: ld must be at least K");
  if (a->steps < 2 || a->steps > PCK_MAX_STEPS) return hm_set_error(HM_ERR_ARG, "hm_pck_auc: steps must be in 2..256");
  if (!(a->val_min < a->val_max) || !(fabs(a->val_min) < INFINITY) || !(fabs(a->val_max) < INFINITY))
    return hm_set_error(HM_ERR_ARG, "hm_pck_auc: val_min < val_max, both finite");
  if (a->chunk_rows < 0) return hm_set_error(HM_ERR_ARG, "hm_pck_auc: chunk_rows must be 0 (default) or positive");
  const size_t need = hm_pck_auc_workspace_bytes(a->K, a->steps);
  if (!a->workspace || a->workspace_bytes < need) return hm_set_error(HM_ERR_ARG, "hm_pck_auc: workspace null or too small");
  if (((uintptr_t)a->workspace & 7) || ((uintptr_t)a->err & 3)) return hm_set_error(HM_ERR_ARG, "hm_pck_auc: workspace must be 8-byte, err 4-byte aligned");
  PckParams p;
  p.err = a->err; p.N = a->N; p.K = a->K; p.ld = a->ld; p.T = a->steps;
  p.start = a->val_min; p.stop = a->val_max;
  p.step = (a->val_max - a->val_min) / (double)(a->steps - 1);
  if (!(p.step > 0.0)) return hm_set_error(HM_ERR_ARG, "hm_pck_auc: val_max - val_min underflows over the steps");
  p.chunk = pck_chunk_rows(a->N, a->chunk_rows);
  p.counts = (unsigned long long*)a->workspace;
  p.pck = a->pck; p.auc = a->auc; p.mean_auc = a->mean_auc; p.curve = a->curve; p.thr_out = a->thresholds;
  hipStream_t s = (hipStream_t)stream_;
  if (hipMemsetAsync(a->workspace, 0, need, s) != hipSuccess) return hm_set_error(HM_ERR_HIP, "hm_pck_auc: hipMemsetAsync failed");
  const unsigned gx = (unsigned)(((long long)a->K + PCK_KT - 1) / PCK_KT);
  const unsigned gy = (unsigned)((a->N + p.chunk - 1) / p.chunk);
  HmProfScope prof(HM_K_OTHER, 1, (int)(a->N > 0x7fffffff ? 0x7fffffff : a->N), a->K, a->steps, s);
  hipLaunchKernelGGL(pck_hist_kernel, dim3(gx, gy), dim3(PCK_KT * PCK_ROWS), 0, s, p);
  const int rc = hm_check_launch("hm_pck_auc (histogram)");
  if (rc != HM_OK) return rc;
  hipLaunchKernelGGL(pck_finish_kernel, dim3(1), dim3(PCK_FINISH_THREADS), 0, s, p);
  return hm_check_launch("hm_pck_auc (finish)");
}
