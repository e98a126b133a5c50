// hm_pose_eval - the hand metrics of hamer/utils/pose_utils.py: the batched similarity Procrustes of
// compute_similarity_transform (:9-58), reconstruction_error (:60-71) and the two means of eval_pose (:73-87), with the root
// subtraction and keypoint selection of Evaluator.__call__ (:163-168), in one launch for the whole batch.
//
// One wave owns one hand (4 hands per 256-thread workgroup).  Lane l holds points l, l + 64, ... (16 at most: P <= 1024) in
// registers, so pred and gt are read from memory once.  Every sum over points -- the centroids, var1, K = X1 X2^T, the two
// error sums -- is a per-lane fp64 sum in ascending point order followed by an xor butterfly (32, 16, .. 1): the order depends
// on P and the mask alone, never on B or the hand's place in the batch, and there are no atomics.  The 3 x 3 solve runs in
// fp64 in every lane (the butterfly leaves all lanes with the same bits).  Outputs are rounded to fp32 once, at the store.
//
// The rotation.  pose_utils.py:38-46 takes K = U S V^T and R = V diag(1, 1, sign det(U V^T)) U^T.  With the singular values
// in descending order that is  R = v1 u1^T + v2 u2^T + (v1 x v2)(u1 x u2)^T : det(U) u3 = u1 x u2 and det(V) v3 = v1 x v2, so
// the third term is the reference's sign-fixed one and only the two leading singular pairs are needed.  They come from a
// one-sided Jacobi SVD (Hestenes): columns of K V are rotated until they are orthogonal; their norms are the singular values.
// A planar set (sigma3 = 0) needs nothing special; a collinear one (sigma2 = 0, N = 2) gets any unit u2 orthogonal to u1, which
// fits exactly as every completion does; K = 0 (coincident gt points) takes R = I, as torch.svd's U = V = I gives.
#include <math.h>
#include <stdio.h>
#include "common.h"
#include "hamer_hip_internal.h"

namespace {

constexpr int MAXC = 16;                           // 64-point chunks: P <= 1024

struct PoseEvalParams {
  const float* pred; const float* gt;
  int B, P, gt_stride, root, n_sel;
  uint64_t sel[MAXC];                              // never all zero here: the host has expanded "all points"
  float* err; float* pa_err; float* aligned; float* transform;
};

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

// one Hestenes rotation of columns p, q of A (= K V so far) and of V; false when they are already orthogonal (or not numbers)
__device__ __forceinline__ bool jacobi_pair(double A[3][3], double V[3][3], int p, int q) {
  const double al = A[0][p] * A[0][p] + A[1][p] * A[1][p] + A[2][p] * A[2][p];
  const double be = A[0][q] * A[0][q] + A[1][q] * A[1][q] + A[2][q] * A[2][q];
  const double ga = A[0][p] * A[0][q] + A[1][p] * A[1][q] + A[2][p] * A[2][q];
  if (!(fabs(ga) > 2e-16 * sqrt(al * be)) || !(fabs(ga) > 0.0)) return false;
  const double zeta = (be - al) / (2.0 * ga);
  const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
  const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
  if (!(s == s) || s == 0.0) return false;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const double ap = A[i][p], aq = A[i][q], vp = V[i][p], vq = V[i][q];
    A[i][p] = c * ap - s * aq; A[i][q] = s * ap + c * aq;
    V[i][p] = c * vp - s * vq; V[i][q] = s * vp + c * vq;
  }
  return true;
}

__device__ __forceinline__ void cross3(const double* a, const double* b, double* o) {
  o[0] = a[1] * b[2] - a[2] * b[1]; o[1] = a[2] * b[0] - a[0] * b[2]; o[2] = a[0] * b[1] - a[1] * b[0];
}

// R of pose_utils.py:38-46 from K (K[i][j] = sum_n X1[i][n] X2[j][n])
__device__ void procrustes_rotation(const double K[3][3], double R[3][3]) {
  double A[3][3], V[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) { A[i][j] = K[i][j]; V[i][j] = i == j ? 1.0 : 0.0; }
  for (int sweep = 0; sweep < 30; ++sweep) {
    bool any = jacobi_pair(A, V, 0, 1);
    any = jacobi_pair(A, V, 0, 2) || any;
    any = jacobi_pair(A, V, 1, 2) || any;
    if (!any) break;
  }
  double n2[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) n2[j] = A[0][j] * A[0][j] + A[1][j] * A[1][j] + A[2][j] * A[2][j];
  // the two largest columns, in order (ties: the lower index first)
  int i1 = 0;
  if (n2[1] > n2[i1]) i1 = 1;
  if (n2[2] > n2[i1]) i1 = 2;
  int i2 = i1 == 0 ? 1 : 0;
  const int other = 3 - i1 - i2;
  if (n2[other] > n2[i2]) i2 = other;
  double a1[3], a2[3], v1[3], v2[3], u1[3], u2[3], v3[3], u3[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {       // (runtime column index on a register array: select, never a scratch access)
    a1[i] = i1 == 0 ? A[i][0] : i1 == 1 ? A[i][1] : A[i][2]; v1[i] = i1 == 0 ? V[i][0] : i1 == 1 ? V[i][1] : V[i][2];
    a2[i] = i2 == 0 ? A[i][0] : i2 == 1 ? A[i][1] : A[i][2]; v2[i] = i2 == 0 ? V[i][0] : i2 == 1 ? V[i][1] : V[i][2];
  }
  const double s1sq = i1 == 0 ? n2[0] : i1 == 1 ? n2[1] : n2[2];
  if (s1sq == 0.0) {
    // K = 0 with finite inputs (the selected gt points coincide, e.g. an annotation stored as zeros): torch.svd of a zero
    // matrix returns U = V = I, so the reference's R is I (then scale = 0 and S1_hat = mu2, all finite)
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) R[i][j] = i == j ? 1.0 : 0.0;
    return;
  }
  const double s1 = sqrt(s1sq);
#pragma unroll
  for (int i = 0; i < 3; ++i) u1[i] = a1[i] / s1;
  const double d = a2[0] * u1[0] + a2[1] * u1[1] + a2[2] * u1[2];
#pragma unroll
  for (int i = 0; i < 3; ++i) a2[i] -= d * u1[i];
  const double m2 = a2[0] * a2[0] + a2[1] * a2[1] + a2[2] * a2[2];
  if (m2 > 1e-28 * s1sq) {
    const double m = sqrt(m2);
#pragma unroll
    for (int i = 0; i < 3; ++i) u2[i] = a2[i] / m;
  } else if (m2 == m2 && s1sq == s1sq) {                                // collinear: any unit vector orthogonal to u1
    const double ax = fabs(u1[0]), ay = fabs(u1[1]), az = fabs(u1[2]);
    double e[3] = {0.0, 0.0, 0.0};
    if (ax <= ay && ax <= az) e[0] = 1.0; else if (ay <= az) e[1] = 1.0; else e[2] = 1.0;
    cross3(u1, e, u2);
    const double m = sqrt(u2[0] * u2[0] + u2[1] * u2[1] + u2[2] * u2[2]);
#pragma unroll
    for (int i = 0; i < 3; ++i) u2[i] /= m;
  } else {
#pragma unroll
    for (int i = 0; i < 3; ++i) u2[i] = NAN;
  }
  cross3(u1, u2, u3);
  cross3(v1, v2, v3);
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) R[i][j] = v1[i] * u1[j] + v2[i] * u2[j] + v3[i] * u3[j];
}

__global__ __launch_bounds__(256) void pose_eval_kernel(const PoseEvalParams p) {
  const int lane = threadIdx.x & 63;
  const int hand = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (hand >= p.B) return;                                              // (no barrier below: a wave may leave alone)
  const float* __restrict__ pr = p.pred + (size_t)hand * p.P * 3;
  const float* __restrict__ gr = p.gt + (size_t)hand * p.P * p.gt_stride;
  float r1[3] = {0.0f, 0.0f, 0.0f}, r2[3] = {0.0f, 0.0f, 0.0f};
  if (p.root >= 0) {
#pragma unroll
    for (int k = 0; k < 3; ++k) { r1[k] = pr[(size_t)p.root * 3 + k]; r2[k] = gr[(size_t)p.root * p.gt_stride + k]; }
  }
  const int nch = (p.P + 63) >> 6;
  const double inv_n = 1.0 / (double)p.n_sel;

  // ---- the only read of the inputs: this lane's selected points, root subtracted in fp64 at every use
  float x[MAXC][3], y[MAXC][3];
  double s1[3] = {0.0, 0.0, 0.0}, s2[3] = {0.0, 0.0, 0.0}, es = 0.0;
#pragma unroll
  for (int c = 0; c < MAXC; ++c) {
    const bool on = c < nch && ((p.sel[c] >> lane) & 1ull);
#pragma unroll
    for (int k = 0; k < 3; ++k) { x[c][k] = 0.0f; y[c][k] = 0.0f; }
    if (on) {
      const int q = c * 64 + lane;                                      // < P: the host refuses a bit at or past P
      double d2 = 0.0;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        x[c][k] = pr[(size_t)q * 3 + k];
        y[c][k] = gr[(size_t)q * p.gt_stride + k];
        const double a = (double)x[c][k] - (double)r1[k], b = (double)y[c][k] - (double)r2[k];
        s1[k] += a; s2[k] += b;
        d2 += (a - b) * (a - b);
      }
      es += sqrt(d2);
    }
  }
  es = wave_sum(es);
  if (p.err && lane == 0) p.err[hand] = (float)(es * inv_n);
  if (!p.pa_err && !p.aligned && !p.transform) return;

  double mu1[3], mu2[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) { mu1[k] = wave_sum(s1[k]) * inv_n; mu2[k] = wave_sum(s2[k]) * inv_n; }

  // ---- var1 and K = X1 X2^T
  double var1 = 0.0, K[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
#pragma unroll
  for (int c = 0; c < MAXC; ++c) {
    const bool on = c < nch && ((p.sel[c] >> lane) & 1ull);
    if (on) {
      double a[3], b[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        a[k] = ((double)x[c][k] - (double)r1[k]) - mu1[k];
        b[k] = ((double)y[c][k] - (double)r2[k]) - mu2[k];
        var1 += a[k] * a[k];
      }
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) K[i][j] += a[i] * b[j];
    }
  }
  var1 = wave_sum(var1);
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) K[i][j] = wave_sum(K[i][j]);

  // ---- R, scale, t (pose_utils.py:37-53)
  double R[3][3], scale, t[3];
  if (es == 0.0 && var1 > 0.0) {
    // pred equals gt in every selected point: the identity fits exactly and is taken as it is, so that comparing a result
    // with itself reports exactly 0 and not the solver's 1e-17 (wave-uniform: es and var1 are the same bits in every lane)
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) R[i][j] = i == j ? 1.0 : 0.0;
    scale = 1.0;
  } else {
    procrustes_rotation(K, R);
    double trace = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) trace += R[i][j] * K[j][i];
    scale = trace / var1;
  }
  if (!(fabs(scale) < INFINITY)) {      // var1 == 0 (the reference's 0 / 0) or a non-finite input: every aligned quantity is NaN
    scale = NAN;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) R[i][j] = NAN;
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) t[i] = mu2[i] - scale * (R[i][0] * mu1[0] + R[i][1] * mu1[1] + R[i][2] * mu1[2]);

  // ---- S1_hat = scale R x + t and its distance to gt
  double ps = 0.0;
  int rank0 = 0;                                                        // selected points below this chunk
  float* __restrict__ al = p.aligned ? p.aligned + (size_t)hand * p.n_sel * 3 : nullptr;
#pragma unroll
  for (int c = 0; c < MAXC; ++c) {
    const uint64_t bits = c < nch ? p.sel[c] : 0ull;
    if ((bits >> lane) & 1ull) {
      double a[3], d2 = 0.0;
#pragma unroll
      for (int k = 0; k < 3; ++k) a[k] = (double)x[c][k] - (double)r1[k];
      const int rank = rank0 + __popcll(bits & ((1ull << lane) - 1ull));
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const double h = scale * (R[i][0] * a[0] + R[i][1] * a[1] + R[i][2] * a[2]) + t[i];
        const double b = (double)y[c][i] - (double)r2[i];
        d2 += (h - b) * (h - b);
        if (al) al[(size_t)rank * 3 + i] = (float)h;
      }
      ps += sqrt(d2);
    }
    rank0 += __popcll(bits);
  }
  ps = wave_sum(ps);
  if (lane == 0) {
    if (p.pa_err) p.pa_err[hand] = (float)(ps * inv_n);
    if (p.transform) {
      float* tr = p.transform + (size_t)hand * 13;
      tr[0] = (float)scale;
#pragma unroll
      for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) tr[1 + i * 3 + j] = (float)R[i][j];
        tr[10 + i] = (float)t[i];
      }
    }
  }
}

}  // namespace

extern "C" int hm_pose_eval(const hm_pose_eval_args* a, void* stream_) {
  if (!a) return hm_set_error(HM_ERR_ARG, "hm_pose_eval: null args");
  if (!a->pred || !a->gt) return hm_set_error(HM_ERR_ARG, "hm_pose_eval: null pred or gt");
  if (a->B <= 0) return hm_set_error(HM_ERR_ARG, "hm_pose_eval: B must be positive");
  if (a->P < 1 || a->P > 64 * MAXC) return hm_set_error(HM_ERR_ARG, "hm_pose_eval: P must be in 1..1024");
  if (a->gt_stride != 3 && a->gt_stride != 4) return hm_set_error(HM_ERR_ARG, "hm_pose_eval: gt_stride must be 3 or 4");
  if (a->root < -1 || a->root >= a->P) return hm_set_error(HM_ERR_ARG, "hm_pose_eval: root must be -1 or an index into P");
  if (!a->err && !a->pa_err && !a->aligned && !a->transform) return hm_set_error(HM_ERR_ARG, "hm_pose_eval: no output requested");
  if (((uintptr_t)a->pred & 3) || ((uintptr_t)a->gt & 3)) return hm_set_error(HM_ERR_ARG, "hm_pose_eval: pred and gt must be 4-byte aligned");
  PoseEvalParams p;
  p.pred = a->pred; p.gt = a->gt; p.B = a->B; p.P = a->P; p.gt_stride = a->gt_stride; p.root = a->root;
  p.err = a->err; p.pa_err = a->pa_err; p.aligned = a->aligned; p.transform = a->transform;
  int n_sel = 0;
  for (int c = 0; c < MAXC; ++c) {
    const int lo = c * 64;
    const uint64_t valid = a->P >= lo + 64 ? ~0ull : a->P > lo ? ((1ull << (a->P - lo)) - 1ull) : 0ull;
    if (a->sel[c] & ~valid) return hm_set_error(HM_ERR_ARG, "hm_pose_eval: sel has a bit at or past P");
    p.sel[c] = a->sel[c];
    n_sel += __builtin_popcountll(a->sel[c]);
  }
  if (n_sel == 0) {                                                     // all zero = all P points
    for (int c = 0; c < MAXC; ++c) {
      const int lo = c * 64;
      p.sel[c] = a->P >= lo + 64 ? ~0ull : a->P > lo ? ((1ull << (a->P - lo)) - 1ull) : 0ull;
    }
    n_sel = a->P;
  }
  p.n_sel = n_sel;
  const unsigned grid = (unsigned)(((long long)a->B + 3) / 4);
  HmProfScope prof(HM_K_OTHER, 0, a->B, a->P, n_sel, (hipStream_t)stream_);
  hipLaunchKernelGGL(pose_eval_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream_, p);
  return hm_check_launch("hm_pose_eval");
}
