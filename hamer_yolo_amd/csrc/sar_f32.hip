// The SAR hand-mesh head's three GEMM shapes in fp32 (the precise route of EstimateRGB: the reference runs the head in fp32,
// rootnet/Model_RGB.py:318-340).  Same layouts and epilogues as their f16 counterparts in sar.hip:
//   SAIGB  : NT, M = 6224 channels, N = 64 * B positions, K = 512; the epilogue scatters to node-major [778][B][544] and
//            writes the template and zero columns;
//   L . X  : NN, M = K = 778 (Laplacian row stride ldl), N = B * C, the [K][N] operand row-major;
//   fc     : NT over 778 * B rows; LeakyReLU(0.1) (layer 0) or raw logits (layer 1), fp32 out.
// v_mfma_f32_32x32x2_f32 (cdna_hip_programming.md §3 'FP32-input MFMA'): f32 in, f32 accumulate, bit-for-bit a k-ordered fmaf
// chain, 64 cycles issue and dependent latency; 128 x 128 tiles of four 64 x 64 waves (2 x 2 independent 32 x 32 accumulators
// per wave keep the pipe busy from one wave per SIMD), K in stages of 32 through a double-buffered LDS tile, the next stage's
// global loads in flight while the MFMAs run (conv_f32.hip's scheme).
//
// Numerics contract: every output is (bias +) ONE sum over k = 0 .. K-1 in a fixed order -- within a stage of 32, for each
// group g of 8, k-slot 0 of the MFMA takes 8g + e and k-slot 1 takes 8g + 4 + e, e = 0..3 -- with no split-K and no
// tile- or batch-dependent reduction.  A hand's numbers are the same bits alone and inside any batch.  For L . X the rows of
// the [K][N] operand at or past kreal = 778 are loaded as zeros, so what lies in memory there never contributes (0 * garbage
// could be NaN in fp32); the Laplacian's columns there are zero by contract.  Rows past M and columns past N read zeros and
// are never stored.
#include <math.h>
#include "common.h"
#include "hamer_hip_internal.h"

namespace {

typedef __attribute__((ext_vector_type(16))) float f32x16_t;

constexpr int NV = 778;
constexpr int KG = 544;             // SAIGB row: 512 features + 3 template + 29 zeros
constexpr int BM = 128, BN = 128, BK = 32;
constexpr int LDK = BK + 4;         // LDS row stride (floats) of the K-contiguous [128][32] images: 144 B, 16-byte aligned rows
constexpr int LDN = BN + 4;         // LDS row stride (floats) of the NN [32][128] image
constexpr int STAGE = BM * LDK + BN * LDK;   // floats per LDS buffer (the NN image, 32 x 132, fits in the B part)
constexpr int LDS_BYTES = 2 * STAGE * 4;     // 73,728 B: double-buffered, above the 64 KiB static limit

enum { G_SAIGB = 0, G_MIX = 1, G_FC_LEAKY = 2, G_FC_LOGITS = 3 };

struct GemmF32 {
  const float* A;      // [M][lda], K contiguous
  const float* B;      // NT: [N][ldb] K contiguous;  MIX: [kreal][ldb] N contiguous
  float* C;
  const float* bias;   // SAIGB: [M];  FC: [N]
  const float* tmpl;   // SAIGB: [778][3]
  int M, N, K, kreal, lda, ldb, ldc, hands;
};

__device__ __forceinline__ float leaky(float x) { return x > 0.f ? x : 0.1f * x; }

template <int MODE>
__global__ __launch_bounds__(256) void sar_gemm_f32_kernel(GemmF32 P) {
  constexpr bool NN = MODE == G_MIX;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave & 1, wn = wave >> 1;
  const int m0 = blockIdx.y * BM, n0 = blockIdx.x * BN;
  const int q = tid & 7, r0 = tid >> 3;                 // K-contiguous images: float4 q of row r0 + 32 i
  const int nq = tid & 31, kr0 = tid >> 5;              // NN image: float4 nq of k row kr0 + 8 i

  f32x4_t ra[4], rb[4];
  auto fetch = [&](int kb) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int m = m0 + r0 + 32 * i, k = kb + 4 * q;   // (L . X: the float4 at 776 holds the Laplacian's zero columns 778, 779)
      ra[i] = f32x4_t{0.f, 0.f, 0.f, 0.f};
      if (m < P.M && k < P.kreal) ra[i] = *(const f32x4_t*)(P.A + (size_t)m * P.lda + k);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      rb[i] = f32x4_t{0.f, 0.f, 0.f, 0.f};
      if constexpr (NN) {
        const int k = kb + kr0 + 8 * i, n = n0 + 4 * nq;
        if (k < P.kreal && n < P.N) rb[i] = *(const f32x4_t*)(P.B + (size_t)k * P.ldb + n);
      } else {
        const int n = n0 + r0 + 32 * i, k = kb + 4 * q;
        if (n < P.N && k < P.kreal) rb[i] = *(const f32x4_t*)(P.B + (size_t)n * P.ldb + k);
      }
    }
  };
  auto stash = [&](int buf) {
    float* s = smem + buf * STAGE;
#pragma unroll
    for (int i = 0; i < 4; ++i) *(f32x4_t*)(s + (r0 + 32 * i) * LDK + 4 * q) = ra[i];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if constexpr (NN) *(f32x4_t*)(s + BM * LDK + (kr0 + 8 * i) * LDN + 4 * nq) = rb[i];
      else *(f32x4_t*)(s + BM * LDK + (r0 + 32 * i) * LDK + 4 * q) = rb[i];
    }
  };

  f32x16_t acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  // operand maps of 32x32x2: lane l holds A[row l & 31][k-slot l >> 5] and B[k-slot l >> 5][col l & 31]
  const int h = lane >> 5, l32 = lane & 31;
  const int arow = (wm * 64 + l32) * LDK + 4 * h;
  const int brow = BM * LDK + (wn * 64 + l32) * LDK + 4 * h;       // NT
  const int bcol = BM * LDK + 4 * h * LDN + wn * 64 + l32;          // NN: k row 8g + 4h + e, column wn*64 + 32j + l32
  const int nk = (P.K + BK - 1) / BK;
  fetch(0);
  stash(0);
  __syncthreads();
  for (int st = 0; st < nk; ++st) {
    const int cur = st & 1;
    if (st + 1 < nk) fetch((st + 1) * BK);
    const float* s = smem + cur * STAGE;
#pragma unroll
    for (int g = 0; g < BK / 8; ++g) {
      f32x4_t av[2], bv[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) av[i] = *(const f32x4_t*)(s + arow + i * 32 * LDK + 8 * g);
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        if constexpr (NN) {
#pragma unroll
          for (int e = 0; e < 4; ++e) bv[j][e] = s[bcol + (8 * g + e) * LDN + 32 * j];
        } else {
          bv[j] = *(const f32x4_t*)(s + brow + j * 32 * LDK + 8 * g);
        }
      }
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i][e], bv[j][e], acc[i][j], 0, 0, 0);
    }
    if (st + 1 < nk) stash(cur ^ 1);
    __syncthreads();
  }

  // 32x32 C/D map: column (n) = lane & 31, row (m) = (r & 3) + 8 (r >> 2) + 4 (lane >> 5); 32 lanes store 128 contiguous bytes
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int n = n0 + wn * 64 + j * 32 + l32;
    if (n >= P.N) continue;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = m0 + wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
        if (m >= P.M) continue;
        const float v = acc[i][j][r];
        if constexpr (MODE == G_SAIGB) {
          const int node = m >> 3, b = n >> 6, p = n & 63;
          float* row = P.C + ((size_t)node * P.hands + b) * KG;
          row[(m & 7) * 64 + p] = leaky(v + P.bias[m]);
          if ((m & 7) == 0 && p < KG - 512) row[512 + p] = p < 3 ? P.tmpl[node * 3 + p] : 0.f;
        } else if constexpr (MODE == G_MIX) {
          P.C[(size_t)m * P.ldc + n] = v;
        } else if constexpr (MODE == G_FC_LEAKY) {
          P.C[(size_t)m * P.ldc + n] = leaky(v + P.bias[n]);
        } else {
          P.C[(size_t)m * P.ldc + n] = v + P.bias[n];
        }
      }
  }
}

template <int MODE> int launch(const GemmF32& p, hipStream_t s, const char* what) {
  static HmLdsOnce lds_once;
  auto kern = sar_gemm_f32_kernel<MODE>;
  if (const int rc = lds_once.ensure((const void*)kern, LDS_BYTES, what)) return rc;
  HmProfScope prof(HM_K_GEMM, 120 + MODE, p.M, p.N, p.K, s);
  hipLaunchKernelGGL(kern, dim3((p.N + BN - 1) / BN, (p.M + BM - 1) / BM), dim3(256), LDS_BYTES, s, p);
  return hm_check_launch(what);
}

bool misaligned16(const void* p) { return ((uintptr_t)p & 15) != 0; }
bool misaligned4(const void* p) { return ((uintptr_t)p & 3) != 0; }

}  // namespace

extern "C" int hm_sar_saigb_f32(const float* feat, const float* w, const float* bias, const float* tmpl, float* g, int B, void* stream) {
  if (!feat || !w || !bias || !tmpl || !g || B <= 0 || misaligned16(feat) || misaligned16(w) || misaligned4(bias) ||
      misaligned4(tmpl) || misaligned4(g))
    return hm_set_error(HM_ERR_ARG, "hm_sar_saigb_f32: bad arguments (feat / w 16-byte aligned)");
  if ((size_t)NV * B * KG >= (1ull << 31)) return hm_set_error(HM_ERR_ARG, "hm_sar_saigb_f32: batch too large");
  GemmF32 p{w, feat, g, bias, tmpl, 8 * NV, B * 64, 512, 512, 512, 512, 0, B};
  return launch<G_SAIGB>(p, (hipStream_t)stream, "hm_sar_saigb_f32");
}

extern "C" int hm_sar_graph_mix_f32(const float* lap, int ldl, const float* x, int N, float* y, void* stream) {
  if (!lap || !x || !y || N <= 0 || N % 4 != 0 || ldl < NV || ldl % 4 != 0 || misaligned16(lap) || misaligned16(x) || misaligned4(y))
    return hm_set_error(HM_ERR_ARG, "hm_sar_graph_mix_f32: bad arguments (N % 4 == 0, ldl >= 778, ldl % 4 == 0, lap / x 16-byte aligned)");
  if ((size_t)NV * N >= (1ull << 31)) return hm_set_error(HM_ERR_ARG, "hm_sar_graph_mix_f32: N too large");
  GemmF32 p{lap, x, y, nullptr, nullptr, NV, N, ldl, NV, ldl, N, N, 0};
  return launch<G_MIX>(p, (hipStream_t)stream, "hm_sar_graph_mix_f32");
}

extern "C" int hm_sar_linear_f32(const float* x, int M, int K, const float* w, const float* bias, float* y, int N, int logits,
                                 void* stream) {
  if (!x || !w || !bias || !y || M <= 0 || N <= 0 || K <= 0 || K % BK != 0 || (logits != 0 && logits != 1) || misaligned16(x) ||
      misaligned16(w) || misaligned4(bias) || misaligned4(y))
    return hm_set_error(HM_ERR_ARG, "hm_sar_linear_f32: bad arguments (K % 32 == 0, logits 0 or 1, x / w 16-byte aligned)");
  if ((size_t)M * (N > K ? N : K) >= (1ull << 31)) return hm_set_error(HM_ERR_ARG, "hm_sar_linear_f32: problem too large");
  GemmF32 p{x, w, y, bias, nullptr, M, N, K, K, K, K, N, 0};
  return logits ? launch<G_FC_LOGITS>(p, (hipStream_t)stream, "hm_sar_linear_f32")
                : launch<G_FC_LEAKY>(p, (hipStream_t)stream, "hm_sar_linear_f32");
}
