// hm_det_match, hm_det_ap, hm_det_ap_curve - the detector evaluation of yolo/yolov7/test.py (:178-209, the matching of
// predictions to labels) and utils/metrics.py (:18-78 ap_per_class, :81-110 compute_ap), with box_iou of general.py:447-469.
//
// Every fp32 and fp64 operation in this file is a plain IEEE operation in the order written: no FMA contraction (the pragma
// below), no fast-math, correctly rounded division.  The tests compare best_iou bit for bit and AP to 1e-12 on that ground.
//
// The match.  One wave owns one image.  test.py walks the label classes in ascending order and, within a class, the
// predictions in stored order; a prediction looks at its best-IoU target of its own class only (lowest index on a tie), is
// assigned when that IoU exceeds iouv[0] and the target is still free, and never falls back to a second best.  Taken sets of
// different classes are disjoint, so the walk is the same as: target t goes to the FIRST prediction (stored order) whose best
// target is t and whose IoU passes.  That is one parallel pass (lane l scores predictions l, l + 64, ... against the labels held
// in LDS), an LDS atomicMin per passing prediction, and one more parallel pass that writes the outputs.  min is order-free, so
// an image's bytes depend on nothing but the image.  The reference's early stop (:208, every label of the image taken) can
// only fire in the last class and only when no further assignment is possible: it changes no output.
//
// The AP.  One 256-thread workgroup owns one (class, threshold) pair; thread t owns the contiguous slice
// [t * L, (t + 1) * L) of the P sorted predictions, L = ceil(P / 256).  Pass 1 counts the slice's members of the class and its
// true positives, one serial 256-step scan turns them into each slice's starting (tpc, fpc).  No curve is stored:
//   - recall is tpc / (n_l + 1e-16), a monotone function of the integer tpc, so the right-most knot of mrec at or below
//     x101[k] is the last element whose tpc is T_k, the largest integer with T_k / (n_l + 1e-16) <= x101[k] (binary search on
//     the integer, the comparison made in fp64 exactly as np.interp makes it);
//   - the next knot is the (T_k + 1)-th true positive (or the end sentinel), where the envelope is
//     M = max over true positives of rank > T_k of rank / (rank + fpc): pass 2 drops each true positive's precision into the
//     bucket of the largest k with T_k < rank (LDS atomicMax on the bits of a non-negative double) and a suffix maximum over
//     101 buckets gives every M; the envelope at the knot itself is max(T_k / (T_k + fpc at the end of its run), M).
//   - p and r (threshold 0 only) interpolate over -conf: grid point px[m] lies between the last member with conf >= px[m] and
//     the first member with conf < px[m], so every member writes the grid points in (conf, conf of the member before it].
// The workspace is therefore empty; the query exists so the ABI need not change if that stops being true.
#include <math.h>
#include <stdio.h>
#include "common.h"
#include "hamer_hip_internal.h"

#pragma clang fp contract(off)

namespace {

constexpr int MATCH_MAX_STRIDE = 4096, MATCH_MAX_LABELS = 1024, MAX_NIOU = 16;
constexpr int AP_MAX_P = 1 << 30, AP_MAX_NC = 65535, AP_THREADS = 256, NX = 101, NPX = 1000;

// torch.min / torch.max of two values: a NaN on either side is the result
__device__ __forceinline__ float tmin(float a, float b) { return a != a ? a : b != b ? b : (a < b ? a : b); }
__device__ __forceinline__ float tmax(float a, float b) { return a != a ? a : b != b ? b : (a > b ? a : b); }

// general.py:447-469 for one pair, fp32
__device__ __forceinline__ float box_iou1(const float* b1, float area1, const float* b2) {
  const float area2 = (b2[2] - b2[0]) * (b2[3] - b2[1]);
  float w = tmin(b1[2], b2[2]) - tmax(b1[0], b2[0]);
  float h = tmin(b1[3], b2[3]) - tmax(b1[1], b2[1]);
  w = w < 0.0f ? 0.0f : w;                                             // clamp(0): a NaN stays a NaN
  h = h < 0.0f ? 0.0f : h;
  const float inter = w * h;
  return inter / (area1 + area2 - inter);
}

__global__ __launch_bounds__(64) void det_match_kernel(const float* __restrict__ pred, const int* __restrict__ pred_count,
                                                       const float* __restrict__ labels, const int* __restrict__ label_count,
                                                       const float* __restrict__ iouv, int stride, int lmax, int niou,
                                                       uint8_t* __restrict__ correct, float* __restrict__ best_iou,
                                                       int* __restrict__ matched) {
  __shared__ float lab[MATCH_MAX_LABELS * 5];
  __shared__ int first[MATCH_MAX_LABELS];
  const int img = blockIdx.x, lane = threadIdx.x;
  int np = pred_count[img], nl = label_count[img];
  np = np < 0 ? 0 : np > stride ? stride : np;
  nl = nl < 0 ? 0 : nl > lmax ? lmax : nl;
  const float* __restrict__ pr = pred + (size_t)img * stride * 6;
  const float* __restrict__ lb = labels + (size_t)img * lmax * 5;
  uint8_t* __restrict__ co = correct + (size_t)img * stride * niou;
  float* __restrict__ bi = best_iou + (size_t)img * stride;
  int* __restrict__ ma = matched + (size_t)img * stride;
  for (int i = lane; i < nl * 5; i += 64) lab[i] = lb[i];
  for (int t = lane; t < nl; t += 64) first[t] = 0x7fffffff;
  __syncthreads();
  const float thr0 = iouv[0];

  // pass 1: every prediction's best target of its class; bi / ma hold (best IoU, candidate) until pass 2 rewrites ma
  for (int i = lane; i < np; i += 64) {
    float b[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) b[k] = pr[(size_t)i * 6 + k];
    const float area1 = (b[2] - b[0]) * (b[3] - b[1]);
    float best = 0.0f;
    int cand = -1;
    bool nan = false;
    for (int t = 0; t < nl; ++t) {
      if (!(lab[t * 5] == b[5])) continue;
      const float iou = box_iou1(b, area1, &lab[t * 5 + 1]);
      if (iou != iou) nan = true;
      else if (cand < 0 || iou > best) { best = iou; cand = t; }       // strict: the lowest index keeps a tie
    }
    if (nan) { best = NAN; cand = -1; }                                // torch.max hands the NaN on: `ious > iouv[0]` is false
    if (cand >= 0 && !(best > thr0)) cand = -1;
    bi[i] = best;
    ma[i] = cand;
    if (cand >= 0) atomicMin(&first[cand], i);
  }
  __syncthreads();
  // pass 2: the first prediction to ask for a target has it; rows at or past the count are 0 / 0 / -1
  for (int i = lane; i < stride; i += 64) {
    float best = 0.0f;
    int m = -1;
    if (i < np) {
      best = bi[i];
      m = ma[i];
      if (m >= 0 && first[m] != i) m = -1;
    } else {
      bi[i] = 0.0f;
    }
    ma[i] = m;
    for (int j = 0; j < niou; ++j) co[(size_t)i * niou + j] = (m >= 0 && best > iouv[j]) ? 1 : 0;
  }
}

// ---- shared by hm_det_ap and hm_det_ap_curve -------------------------------------------------------------------------------

// np.interp between knot j and j + 1: fp[j] + (x - xp[j]) * ((fp[j+1] - fp[j]) / (xp[j+1] - xp[j]))
__device__ __forceinline__ double interp_between(double x, double xj, double xj1, double fj, double fj1) {
  const double slope = (fj1 - fj) / (xj1 - xj);
  return fj + (x - xj) * slope;
}

// np.trapz(y, x) over the 101 points: the terms d * (y[k+1] + y[k]) / 2.0 summed the way numpy's pairwise sum adds 100 values
// (eight strided partial sums, a fixed tree over them, the last four values in order)
__device__ double trapz101(const double* y, const double* x) {
  double r[8];
#pragma unroll
  for (int m = 0; m < 8; ++m) r[m] = (x[m + 1] - x[m]) * (y[m + 1] + y[m]) / 2.0;
  for (int i = 8; i < 96; i += 8)
#pragma unroll
    for (int m = 0; m < 8; ++m) r[m] += (x[i + m + 1] - x[i + m]) * (y[i + m + 1] + y[i + m]) / 2.0;
  double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
  for (int i = 96; i < 100; ++i) res += (x[i + 1] - x[i]) * (y[i + 1] + y[i]) / 2.0;
  return res;
}

__global__ __launch_bounds__(AP_THREADS) void det_ap_kernel(const uint8_t* __restrict__ tp, const float* __restrict__ conf,
                                                            const float* __restrict__ pred_cls, int P,
                                                            const float* __restrict__ classes, const int* __restrict__ n_labels,
                                                            int niou, const double* __restrict__ x101,
                                                            const double* __restrict__ px, int v5_metric,
                                                            double* __restrict__ ap, double* __restrict__ pout,
                                                            double* __restrict__ rout) {
  __shared__ int s_n[AP_THREADS], s_tp[AP_THREADS];                    // per slice: members, true positives -> exclusive sums
  __shared__ float s_prev[AP_THREADS];                                 // conf of the last member before the slice
  __shared__ int s_has[AP_THREADS];
  __shared__ int s_tot[3];                                             // n_p, ntp, index of the last member
  __shared__ int s_T[NX];
  __shared__ unsigned long long s_bucket[NX];
  __shared__ int s_fnext[NX];                                          // fpc at true positive T_k + 1, stored at the last k of T_k
  __shared__ double s_x[NX], s_y[NX];
  const int ci = blockIdx.x, j = blockIdx.y, t = threadIdx.x;
  const float c = classes[ci];
  const int n_l = n_labels[ci];
  const long long L = ((long long)P + AP_THREADS - 1) / AP_THREADS;
  const long long lo = (long long)t * L < P ? (long long)t * L : P, hi = lo + L < P ? lo + L : P;

  int n = 0, ntp_t = 0, last = -1;
  for (long long i = lo; i < hi; ++i)
    if (pred_cls[i] == c) { ++n; ntp_t += tp[(size_t)i * niou + j] ? 1 : 0; last = (int)i; }
  s_n[t] = n; s_tp[t] = ntp_t; s_has[t] = last;
  if (t < NX) { s_x[t] = x101[t]; s_bucket[t] = 0ull; s_fnext[t] = 0; }
  __syncthreads();
  if (t == 0) {
    int an = 0, at = 0, lastm = -1;
    for (int q = 0; q < AP_THREADS; ++q) {
      const int qn = s_n[q], qt = s_tp[q], ql = s_has[q];
      s_n[q] = an; s_tp[q] = at;
      s_has[q] = lastm >= 0; s_prev[q] = lastm >= 0 ? conf[lastm] : 0.0f;
      an += qn; at += qt;
      if (ql >= 0) lastm = ql;
    }
    s_tot[0] = an; s_tot[1] = at; s_tot[2] = lastm;
  }
  __syncthreads();
  const int n_p = s_tot[0], ntp = s_tot[1], nfp = n_p - ntp, lastm = s_tot[2];
  if (n_p == 0 || n_l <= 0) {                                          // metrics.py:48-49: the rows stay zero
    if (t == 0) ap[(size_t)ci * niou + j] = 0.0;
    if (j == 0)
      for (int m = t; m < NPX; m += AP_THREADS) { pout[(size_t)ci * NPX + m] = 0.0; rout[(size_t)ci * NPX + m] = 0.0; }
    return;
  }
  const double nl_eps = (double)n_l + 1e-16;
  if (t < NX) {                                                        // T_k: t / nl_eps is monotone in the integer t
    const double x = s_x[t];
    int a = 0, b = ntp;                                                // 0 / nl_eps = 0 <= x always (x101 >= 0)
    while (a < b) {
      const int mid = a + (b - a + 1) / 2;
      if ((double)mid / nl_eps <= x) a = mid; else b = mid - 1;
    }
    s_T[t] = a;
  }
  if (j == 0)                                                          // left of the first knot: np.interp's `left`
    for (int m = t; m < NPX; m += AP_THREADS) { pout[(size_t)ci * NPX + m] = 1.0; rout[(size_t)ci * NPX + m] = 0.0; }
  __syncthreads();

  // pass 2
  int tpc = s_tp[t], fpc = s_n[t] - s_tp[t];
  bool has_prev = s_has[t] != 0;
  float prev_conf = s_prev[t];
  for (long long i = lo; i < hi; ++i) {
    if (!(pred_cls[i] == c)) continue;
    const bool is_tp = tp[(size_t)i * niou + j] != 0;
    const int tpc0 = tpc, fpc0 = fpc;
    if (is_tp) ++tpc; else ++fpc;
    if (is_tp) {
      // the largest k with T_k < tpc (k = 0 always qualifies: T_0 = 0 because x101[0] = 0 admits no positive recall ...
      // unless the grid starts above 0, in which case ranks at or below T_0 belong to no bucket)
      int a = -1, b = NX - 1;
      while (a < b) {
        const int mid = a + (b - a + 1) / 2;
        if (s_T[mid] < tpc) a = mid; else b = mid - 1;
      }
      if (a >= 0) {
        const double prec = (double)tpc / (double)(tpc + fpc);
        atomicMax(&s_bucket[a], (unsigned long long)__double_as_longlong(prec));
        if (s_T[a] + 1 == tpc) s_fnext[a] = fpc;
      }
    }
    if (j == 0) {
      const float cf = conf[i];
      if (has_prev) {
        // grid points with conf < px <= prev_conf: knot j is the member before, knot j + 1 this one
        int a = 0, b = NPX;                                            // first m with px[m] > cf
        while (a < b) { const int mid = (a + b) >> 1; if (px[mid] > (double)cf) b = mid; else a = mid + 1; }
        const int m0 = a;
        a = m0; b = NPX;                                               // first m with px[m] > prev_conf
        while (a < b) { const int mid = (a + b) >> 1; if (px[mid] > (double)prev_conf) b = mid; else a = mid + 1; }
        const double xj = -(double)prev_conf, xj1 = -(double)cf;
        const double r0 = (double)tpc0 / nl_eps, r1 = (double)tpc / nl_eps;
        const double p0 = (double)tpc0 / (double)(tpc0 + fpc0), p1 = (double)tpc / (double)(tpc + fpc);
        for (int m = m0; m < a; ++m) {
          const double x = -px[m];
          rout[(size_t)ci * NPX + m] = interp_between(x, xj, xj1, r0, r1);
          pout[(size_t)ci * NPX + m] = interp_between(x, xj, xj1, p0, p1);
        }
      }
      if ((int)i == lastm) {                                           // at or right of the last knot: fp[-1]
        int a = 0, b = NPX;
        while (a < b) { const int mid = (a + b) >> 1; if (px[mid] > (double)cf) b = mid; else a = mid + 1; }
        const double rl = (double)tpc / nl_eps, pl = (double)tpc / (double)(tpc + fpc);
        for (int m = 0; m < a; ++m) { rout[(size_t)ci * NPX + m] = rl; pout[(size_t)ci * NPX + m] = pl; }
      }
      has_prev = true; prev_conf = cf;
    }
  }
  __syncthreads();
  if (t < NX) {
    const int k = t, T = s_T[k];
    const double x = s_x[k];
    const double mrec_end = v5_metric ? 1.0 : (double)ntp / nl_eps + 0.01;
    double y;
    if (x >= mrec_end) {
      y = 0.0;                                                         // mpre[-1]
    } else {
      int rep = k;
      while (rep + 1 < NX && s_T[rep + 1] == T) ++rep;
      unsigned long long mb = 0ull;
      for (int q = k; q < NX; ++q) mb = s_bucket[q] > mb ? s_bucket[q] : mb;
      const double M = T < ntp ? __longlong_as_double((long long)mb) : 0.0;       // mpre[j + 1]
      const int f_last = T < ntp ? s_fnext[rep] : nfp;                 // fpc at the last element of run T
      const double pj = (T == 0 && f_last == 0) ? 1.0 : (double)T / (double)(T + f_last);   // (the leading sentinel is 1)
      const double fj = pj > M ? pj : M;
      const double xj = (double)T / nl_eps, xj1 = T < ntp ? (double)(T + 1) / nl_eps : mrec_end;
      y = interp_between(x, xj, xj1, fj, M);
    }
    s_y[k] = y;
  }
  __syncthreads();
  if (t == 0) ap[(size_t)ci * niou + j] = trapz101(s_y, s_x);
}

// compute_ap for a given curve: one workgroup; thread t owns a contiguous slice of the n + 2 knots
__global__ __launch_bounds__(AP_THREADS) void det_ap_curve_kernel(const double* __restrict__ recall,
                                                                  const double* __restrict__ precision, int n,
                                                                  const double* __restrict__ x101, int v5_metric,
                                                                  double* __restrict__ ap, double* __restrict__ mpre,
                                                                  double* __restrict__ mrec) {
  __shared__ double s_max[AP_THREADS];
  __shared__ double s_x[NX], s_y[NX];
  const int t = threadIdx.x;
  const long long n2 = (long long)n + 2;
  const long long L = (n2 + AP_THREADS - 1) / AP_THREADS;
  const long long lo = (long long)t * L < n2 ? (long long)t * L : n2, hi = lo + L < n2 ? lo + L : n2;
  const double mrec_end = v5_metric ? 1.0 : recall[n - 1] + 0.01;
  double mx = 0.0;                                                     // (mpre's last value is 0 and precisions are >= 0)
  for (long long i = lo; i < hi; ++i) {
    const double pv = i == 0 ? 1.0 : i == n2 - 1 ? 0.0 : precision[i - 1];
    mrec[i] = i == 0 ? 0.0 : i == n2 - 1 ? mrec_end : recall[i - 1];
    mx = pv > mx ? pv : mx;
  }
  s_max[t] = mx;
  if (t < NX) s_x[t] = x101[t];
  __syncthreads();
  if (t == 0) {                                                        // s_max[q] <- the maximum of every slice after q
    double run = 0.0;
    for (int q = AP_THREADS - 1; q >= 0; --q) { const double v = s_max[q]; s_max[q] = run; run = v > run ? v : run; }
  }
  __syncthreads();
  double run = s_max[t];
  for (long long i = hi - 1; i >= lo; --i) {
    const double pv = i == 0 ? 1.0 : i == n2 - 1 ? 0.0 : precision[i - 1];
    run = pv > run ? pv : run;
    mpre[i] = run;
  }
  __syncthreads();                                                     // (one workgroup: its own global writes are visible)
  if (t < NX) {
    const double x = s_x[t];
    double y;
    if (x >= mrec[n2 - 1]) {
      y = mpre[n2 - 1];
    } else if (x < mrec[0]) {
      y = mpre[0];
    } else {
      long long a = 0, b = n2 - 2;                                     // the right-most knot at or below x
      while (a < b) { const long long mid = a + (b - a + 1) / 2; if (mrec[mid] <= x) a = mid; else b = mid - 1; }
      y = interp_between(x, mrec[a], mrec[a + 1], mpre[a], mpre[a + 1]);
    }
    s_y[t] = y;
  }
  __syncthreads();
  if (t == 0) *ap = trapz101(s_y, s_x);
}

}  // namespace

extern "C" int hm_det_match(const float* pred, const int* pred_count, const float* labels, const int* label_count,
                            const float* iouv, int N, int stride, int lmax, int niou, uint8_t* correct, float* best_iou,
                            int* matched, void* stream_) {
  if (!pred || !pred_count || !labels || !label_count || !iouv || !correct || !best_iou || !matched)
    return hm_set_error(HM_ERR_ARG, "hm_det_match: null pointer");
  if (N < 1) return hm_set_error(HM_ERR_ARG, "hm_det_match: N must be positive");
  if (stride < 1 || stride > MATCH_MAX_STRIDE) return hm_set_error(HM_ERR_ARG, "hm_det_match: stride must be in 1..4096");
  if (lmax < 1 || lmax > MATCH_MAX_LABELS) return hm_set_error(HM_ERR_ARG, "hm_det_match: lmax must be in 1..1024");
  if (niou < 1 || niou > MAX_NIOU) return hm_set_error(HM_ERR_ARG, "hm_det_match: niou must be in 1..16");
  HmProfScope prof(HM_K_OTHER, 0, N, stride, lmax, (hipStream_t)stream_);
  hipLaunchKernelGGL(det_match_kernel, dim3((unsigned)N), dim3(64), 0, (hipStream_t)stream_, pred, pred_count, labels,
                     label_count, iouv, stride, lmax, niou, correct, best_iou, matched);
  return hm_check_launch("hm_det_match");
}

static int det_ap_check(int P, int nc, int niou) {
  if (P < 0 || P > AP_MAX_P) return hm_set_error(HM_ERR_ARG, "hm_det_ap: P must be in 0..2^30");
  if (nc < 1 || nc > AP_MAX_NC) return hm_set_error(HM_ERR_ARG, "hm_det_ap: nc must be in 1..65535");
  if (niou < 1 || niou > MAX_NIOU) return hm_set_error(HM_ERR_ARG, "hm_det_ap: niou must be in 1..16");
  return HM_OK;
}

extern "C" size_t hm_det_ap_workspace_bytes(int P, int nc, int niou) {
  (void)P; (void)nc; (void)niou;
  return 0;
}

extern "C" int hm_det_ap(const uint8_t* tp, const float* conf, const float* pred_cls, int P, const float* classes,
                         const int* n_labels, int nc, int niou, const double* x101, const double* px, int v5_metric,
                         double* ap, double* p, double* r, void* workspace, size_t workspace_bytes, void* stream_) {
  (void)workspace; (void)workspace_bytes;
  if (const int rc = det_ap_check(P, nc, niou)) return rc;
  if ((P > 0 && (!tp || !conf || !pred_cls)) || !classes || !n_labels || !x101 || !px || !ap || !p || !r)
    return hm_set_error(HM_ERR_ARG, "hm_det_ap: null pointer");
  HmProfScope prof(HM_K_OTHER, 0, P, nc, niou, (hipStream_t)stream_);
  hipLaunchKernelGGL(det_ap_kernel, dim3((unsigned)nc, (unsigned)niou), dim3(AP_THREADS), 0, (hipStream_t)stream_, tp, conf,
                     pred_cls, P, classes, n_labels, niou, x101, px, v5_metric ? 1 : 0, ap, p, r);
  return hm_check_launch("hm_det_ap");
}

extern "C" int hm_det_ap_curve(const double* recall, const double* precision, int n, const double* x101, int v5_metric,
                               double* ap, double* mpre, double* mrec, void* stream_) {
  if (!recall || !precision || !x101 || !ap || !mpre || !mrec) return hm_set_error(HM_ERR_ARG, "hm_det_ap_curve: null pointer");
  if (n < 1 || n > AP_MAX_P) return hm_set_error(HM_ERR_ARG, "hm_det_ap_curve: n must be in 1..2^30");
  HmProfScope prof(HM_K_OTHER, 0, n, 0, 0, (hipStream_t)stream_);
  hipLaunchKernelGGL(det_ap_curve_kernel, dim3(1), dim3(AP_THREADS), 0, (hipStream_t)stream_, recall, precision, n, x101,
                     v5_metric ? 1 : 0, ap, mpre, mrec);
  return hm_check_launch("hm_det_ap_curve");
}
