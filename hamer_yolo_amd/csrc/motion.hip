// Motion across frames: the symmetric-pair filter of hand tracks and the acceleration of point tracks.
// The rule is stated in include/hamer_hip.h ("Motion"); tests/motion_rule.py restates it in numpy.
//  * smooth_kernel - a workgroup is (tile of 32 frames, track): 256 threads as 32 frames x 8 units, a unit being one rotation
//                (9 doubles) or up to 9 linear channels.  The units go by in passes of 8 (a hand of 16 rotations and 13 channels:
//                three passes); per pass the present frames of the tile and of its halo of R on each side are staged in LDS,
//                (32 + 2 R) frames x 8 units x 72 B, at most 54 KiB.  A thread forms its unit's weighted sum in the rule's order,
//                divides, and for a rotation runs the 12 Newton steps.  A degenerate rotation raises its frame's flag in LDS;
//                after the last pass the threads of a flagged frame write the unit outputs they own again, as the input's bytes
//                or NaN: that is the one exchange the DEGENERATE decision needs, and the same thread writes the same address
//                both times.
//  * jitter_kernel - a wave per (frame, track): lane l adds the norms of points l, l + 64, ..., then six shuffle steps.
// The weights travel as kernel arguments.  The file is compiled without contraction and every fp64 expression is written in
// the rule's order; a (frame, track) reads its own window only, so its bytes do not depend on N, S or the tile it falls in.
#include <math.h>
#include <string>
#include "common.h"
#include "hamer_hip_internal.h"

#pragma clang fp contract(off)

namespace {

constexpr int TILE = 32, GROUP = 8, MAX_R = HM_MOTION_MAX_RADIUS, WINDOW = TILE + 2 * MAX_R;
constexpr int STEPS = 12;
constexpr double MIN_DET = 1.0 / 64.0;

struct Weights { double w[MAX_R + 1]; };

int motion_error(const char* entry, const char* what) { return hm_set_error(HM_ERR_ARG, (std::string(entry) + ": " + what).c_str()); }

// The cofactor matrix c of m and its determinant, in the header's order.
__device__ __forceinline__ double cofactors(const double* m, double* c) {
  c[0] = m[4] * m[8] - m[5] * m[7];
  c[1] = m[5] * m[6] - m[3] * m[8];
  c[2] = m[3] * m[7] - m[4] * m[6];
  c[3] = m[2] * m[7] - m[1] * m[8];
  c[4] = m[0] * m[8] - m[2] * m[6];
  c[5] = m[1] * m[6] - m[0] * m[7];
  c[6] = m[1] * m[5] - m[2] * m[4];
  c[7] = m[2] * m[3] - m[0] * m[5];
  c[8] = m[0] * m[4] - m[1] * m[3];
  return (m[0] * c[0] + m[1] * c[1]) + m[2] * c[2];
}

struct SmoothArgs {
  const double* rot;           // [N][S][J][9]
  const double* lin;           // [N][S][C]
  const uint8_t* present;      // [N][S]
  double* rot_out;
  double* lin_out;
  int32_t* status;
  int32_t* pairs;
  int32_t* nearest;
  double* moved;               // [N][S][J]
  int N, S, J, C, R;
};

// The doubles of unit u of row (t, s): a rotation's 9, or the linear channels 9 (u - J) .. of which `n` exist.
__device__ __forceinline__ const double* unit_in(const SmoothArgs& a, size_t row, int u, int& n) {
  if (u < a.J) { n = 9; return a.rot + (row * a.J + u) * 9; }
  const int c0 = (u - a.J) * 9;
  n = min(9, a.C - c0);
  return a.lin + row * a.C + c0;
}
__device__ __forceinline__ double* unit_out(const SmoothArgs& a, size_t row, int u) {
  return u < a.J ? a.rot_out + (row * a.J + u) * 9 : a.lin_out + row * a.C + (size_t)(u - a.J) * 9;
}

// The unit's outputs as the input's bytes (present) or NaN (absent).
__device__ __forceinline__ void write_raw(const SmoothArgs& a, size_t row, int u, bool here) {
  int n;
  const unsigned long long* in = (const unsigned long long*)unit_in(a, row, u, n);
  unsigned long long* out = (unsigned long long*)unit_out(a, row, u);
  const unsigned long long nan = (unsigned long long)__double_as_longlong(__builtin_nan(""));
  for (int e = 0; e < n; ++e) out[e] = here ? in[e] : nan;
  if (u < a.J) a.moved[row * a.J + u] = __builtin_nan("");
}

__global__ __launch_bounds__(256) void smooth_kernel(SmoothArgs a, Weights wt) {
  __shared__ double s_data[WINDOW][GROUP][9];
  __shared__ uint8_t s_here[WINDOW];
  __shared__ unsigned s_mask[TILE];            // bit k - 1: the pair at offset k is used
  __shared__ int s_bad[TILE];
  const int tid = threadIdx.x, f = tid >> 3, g = tid & 7;
  const int s = (int)(blockIdx.x % (unsigned)a.S), t0 = (int)(blockIdx.x / (unsigned)a.S) * TILE;
  const int R = a.R, window = TILE + 2 * R, units = a.J + (a.C + 8) / 9;
  for (int i = tid; i < window; i += 256) {
    const int t = t0 - R + i;
    s_here[i] = (t >= 0 && t < a.N && a.present[(size_t)t * a.S + s] != 0) ? 1 : 0;
  }
  __syncthreads();
  if (tid < TILE) {
    unsigned mask = 0;
    for (int k = 1; k <= R; ++k)
      if (s_here[R + tid - k] && s_here[R + tid + k]) mask |= 1u << (k - 1);
    s_mask[tid] = mask;
    s_bad[tid] = 0;
  }
  __syncthreads();
  const int t = t0 + f;
  const bool live = t < a.N;
  const bool here = s_here[R + f] != 0;
  const unsigned mask = s_mask[f];
  const size_t row = (size_t)(live ? t : 0) * a.S + s;
  for (int u0 = 0; u0 < units; u0 += GROUP) {
    // stage the present frames of the window, 8 units each
    for (int i = tid; i < window * GROUP; i += 256) {
      const int fi = i >> 3, u = u0 + (i & 7);
      if (u < units && s_here[fi]) {
        int n;
        const double* in = unit_in(a, (size_t)(t0 - R + fi) * a.S + s, u, n);
        for (int e = 0; e < n; ++e) s_data[fi][i & 7][e] = in[e];
      }
    }
    __syncthreads();
    const int u = u0 + g;
    if (live && u < units) {
      int n;
      const double* in = unit_in(a, row, u, n);
      if (mask == 0) {
        write_raw(a, row, u, here);
      } else {
        double acc[9], W;
        const double* c = s_data[R + f][g];
        for (int e = 0; e < 9; ++e) acc[e] = (here && e < n) ? wt.w[0] * c[e] : 0.0;
        W = here ? wt.w[0] : 0.0;
        for (int k = 1; k <= R; ++k) {
          if (!((mask >> (k - 1)) & 1u)) continue;
          const double* lo = s_data[R + f - k][g];
          const double* hi = s_data[R + f + k][g];
          const double wk = wt.w[k];
          for (int e = 0; e < 9; ++e)
            if (e < n) acc[e] = acc[e] + wk * (lo[e] + hi[e]);
          W = W + 2.0 * wk;
        }
        double x[9];
        for (int e = 0; e < 9; ++e) x[e] = acc[e] / W;
        double* out = unit_out(a, row, u);
        if (u < a.J) {
          double cf[9];
          const double det = cofactors(x, cf);
          if (!(det >= MIN_DET)) {
            s_bad[f] = 1;                                                // every writer writes 1
            write_raw(a, row, u, here);
          } else {
            for (int it = 0; it < STEPS; ++it) {
              const double d = cofactors(x, cf);
              for (int e = 0; e < 9; ++e) x[e] = (x[e] + cf[e] / d) * 0.5;
            }
            double m = 0.0;
            for (int e = 0; e < 9; ++e) {
              out[e] = x[e];
              const double d = x[e] - in[e];
              m = m + d * d;
            }
            a.moved[row * a.J + u] = here ? m : __builtin_nan("");
          }
        } else {
          for (int e = 0; e < n; ++e) out[e] = x[e];
        }
      }
    }
    __syncthreads();                                                     // the stage is rewritten by the next pass
  }
  const bool bad = s_bad[f] != 0;                                        // complete: the last pass ended with a barrier
  if (!live) return;
  if (bad)
    for (int u = g; u < units; u += GROUP) write_raw(a, row, u, here);
  if (g == 0) {
    const int n_pairs = __popc(mask);
    a.status[row] = bad ? HM_TRACK_DEGENERATE : n_pairs == 0 ? (here ? HM_TRACK_KEPT : HM_TRACK_ABSENT) : (here ? HM_TRACK_SMOOTHED : HM_TRACK_FILLED);
    a.pairs[row] = n_pairs;
    a.nearest[row] = mask ? __ffs(mask) : 0;
  }
}

__global__ __launch_bounds__(256) void jitter_kernel(const double* __restrict__ points, const uint8_t* __restrict__ present,
                                                     long long rows, int N, int S, int P, double* __restrict__ accel) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);          // uniform in the wave
  if (row >= rows) return;
  const int t = (int)(row / S);
  const bool ok = t >= 1 && t + 1 < N && present[row - S] != 0 && present[row] != 0 && present[row + S] != 0;
  if (!ok) {
    if (lane == 0) accel[row] = __builtin_nan("");
    return;
  }
  const size_t step = (size_t)S * P * 3;
  const double* x1 = points + (size_t)row * P * 3;
  const double *x0 = x1 - step, *x2 = x1 + step;
  double v = 0.0;
  for (int p = lane; p < P; p += 64) {
    const double dx = (x0[p * 3] - 2.0 * x1[p * 3]) + x2[p * 3];
    const double dy = (x0[p * 3 + 1] - 2.0 * x1[p * 3 + 1]) + x2[p * 3 + 1];
    const double dz = (x0[p * 3 + 2] - 2.0 * x1[p * 3 + 2]) + x2[p * 3 + 2];
    v = v + sqrt((dx * dx + dy * dy) + dz * dz);
  }
  for (int o = 32; o > 0; o >>= 1) v = v + __shfl_down(v, o);
  if (lane == 0) accel[row] = v / (double)P;
}

}  // namespace

extern "C" int hm_track_smooth(const double* rot, const double* lin, const uint8_t* present, int N, int S, int J, int C,
                               const double* weights_host, int R, double* rot_out, double* lin_out, int32_t* status, int32_t* pairs,
                               int32_t* nearest_pair, double* moved, void* stream_) {
  const char* entry = "hm_track_smooth";
  if (N < 0 || S < 0 || J < 0 || C < 0) return motion_error(entry, "negative count");
  if (R < 0 || R > MAX_R) return motion_error(entry, "the radius must lie in 0 .. 32");
  if (!weights_host) return motion_error(entry, "null weights");
  for (int k = 0; k <= R; ++k)
    if (!(weights_host[k] >= 0.0 && weights_host[k] <= 1.0)) return motion_error(entry, "a weight outside 0 .. 1");
  if (N == 0 || S == 0) return HM_OK;
  if (!present || !status || !pairs || !nearest_pair) return motion_error(entry, "null pointer");
  if (J > 0 && (!rot || !rot_out || !moved)) return motion_error(entry, "null rotations");
  if (C > 0 && (!lin || !lin_out)) return motion_error(entry, "null linear channels");
  if (((uintptr_t)rot | (uintptr_t)lin | (uintptr_t)rot_out | (uintptr_t)lin_out | (uintptr_t)moved) & 7)
    return motion_error(entry, "the fp64 arrays must be 8-byte aligned");
  if (((uintptr_t)status | (uintptr_t)pairs | (uintptr_t)nearest_pair) & 3) return motion_error(entry, "the int32 arrays must be 4-byte aligned");
  if (rot_out == rot || (C > 0 && lin_out == lin)) return motion_error(entry, "never in place: a frame's neighbours read its input");
  const long long blocks = ((long long)N + TILE - 1) / TILE * S;
  if (blocks >= (1ll << 31) || (long long)N * S >= (1ll << 31)) return motion_error(entry, "too many frames x tracks");
  SmoothArgs a;
  a.rot = rot; a.lin = lin; a.present = present; a.rot_out = rot_out; a.lin_out = lin_out; a.status = status; a.pairs = pairs;
  a.nearest = nearest_pair; a.moved = moved; a.N = N; a.S = S; a.J = J; a.C = C; a.R = R;
  Weights wt = {};
  for (int k = 0; k <= R; ++k) wt.w[k] = weights_host[k];
  hipStream_t s = (hipStream_t)stream_;
  HmProfScope prof(HM_K_OTHER, 5, N, S, R, s);
  hipLaunchKernelGGL(smooth_kernel, dim3((unsigned)blocks), dim3(256), 0, s, a, wt);
  return hm_check_launch(entry);
}

extern "C" int hm_track_jitter(const double* points, const uint8_t* present, int N, int S, int P, double* accel, void* stream_) {
  const char* entry = "hm_track_jitter";
  if (N < 0 || S < 0 || P < 0) return motion_error(entry, "negative count");
  if (P > HM_MOTION_MAX_POINTS) return motion_error(entry, "more than 1024 points");
  if (N == 0 || S == 0) return HM_OK;
  if (P == 0) return motion_error(entry, "no points");
  if (!points || !present || !accel) return motion_error(entry, "null pointer");
  if (((uintptr_t)points | (uintptr_t)accel) & 7) return motion_error(entry, "points and accel must be 8-byte aligned");
  const long long rows = (long long)N * S;
  if (rows >= (1ll << 31)) return motion_error(entry, "too many frames x tracks");
  hipStream_t s = (hipStream_t)stream_;
  HmProfScope prof(HM_K_OTHER, 6, N, S, P, s);
  hipLaunchKernelGGL(jitter_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, points, present, rows, N, S, P, accel);
  return hm_check_launch(entry);
}
