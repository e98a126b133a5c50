// hm_gemm_f32: nn.Linear in fp32 operands for the precise HaMeR route (HamerEngine(dtype=torch.float32)) -- the reference's
// fp32 CPU arithmetic (aten::addmm behind vit.py:83-85,:114,:124,:172 and pose_transformer.py:114) on the fp32-input MFMA.
//   C[M][N] = epilogue(X[M][K] . W[N][K]^T), all fp32, row-major, W as nn.Linear stores it.
// v_mfma_f32_32x32x2_f32 (cdna_hip_programming.md section 3 'FP32-input MFMA'): f32 in, f32 accumulate, bit-for-bit a k-ordered
// fmaf chain; 64 cycles issue and dependent latency per SIMD, so the 2 x 2 independent 32x32 accumulators of a wave keep the
// pipe busy from one wave per SIMD.  157 TF/s peak = the f32 vector rate.
//
// Numerics contract (conv_f32.hip's, for a plain GEMM): every output is epilogue(bias + ONE sum over K), the sum being one
// fmaf chain started at zero whose order depends on K only: no split-K, no K groups inside a workgroup, no tile-dependent or
// grid-dependent reduction.  The residual is added behind the accumulation, (acc + bias) + resid, at every size.  An output
// therefore does not depend on the tile shape, the grid, M, or the row's place in the batch: rows computed alone are the same
// bytes as the same rows inside any larger M.
//
// Tile loop: conv_f32.hip's staged loop without the tap arithmetic (the MFMA side of a stage is shared: mfma_f32_tile.h).  256 threads = 4 waves as 2 x 2, a wave owns RB x CB blocks
// of 32x32.  K moves in stages of 32 fp32: every thread fetches its float4 pieces of the next stage into registers (dwordx4
// loads, in flight while the MFMAs run), then writes them to the other half of a double-buffered LDS tile -- one barrier per
// stage.  LDS rows are 32 + 4 floats (144 B): 16-byte aligned for ds_read_b128, and the 32 rows one operand read touches start
// in different banks.  Within a stage the K order is: for each group g of 8 k, lanes 0-31 (k-slot 0 of the MFMA) hold
// k = 8g + e and lanes 32-63 (k-slot 1) hold k = 8g + 4 + e, e = 0..3 the MFMA's index in the group -- the same on both
// operands, and the same as conv_f32.hip, so a 1x1 convolution and this kernel sum in one order.
// Rows past M and columns past N are fetched from the last valid row (finite, never stored): no branches in the loader.
// Tiles walk M fastest inside groups of 8 M-tiles, and the workgroups of one XCD take consecutive tile ids: the 64 workgroups an
// XCD holds at a time form an 8 x 8 square of tiles that shares its X rows and W rows in that XCD's L2.
#include <math.h>
#include <stdio.h>
#include "common.h"
#include "hamer_hip_internal.h"
#include "mfma_f32_tile.h"      // F32_BK, F32_LDK and the MFMA side of the stage loop, shared with conv_f32.hip

namespace {

constexpr int G32_GROUP_M = 8;         // M-tiles per group of the tile walk

struct GemmF32Args {
  const float* X; const float* W; const float* bias; const float* R; float* C;
  int M, N, K, ldx, ldw, ldc, ldr, rmod, tiles_m, tiles_n;
};

enum { G32_BIAS = 0, G32_GELU = 1, G32_RESID = 2 };

template <int RB, int CB>
constexpr int gemm_f32_lds_bytes() { return 2 * (2 * RB * 32 + 2 * CB * 32) * F32_LDK * 4; }

template <int RB, int CB, int EPI>
__global__ __launch_bounds__(256) void gemm_f32_kernel(GemmF32Args a) {
  constexpr int BM = 2 * RB * 32, BN = 2 * CB * 32;
  constexpr int AL = BM / 32, BL = BN / 32;         // float4 pieces per thread and stage: 8 per tile row, 32 rows per pass
  constexpr int STAGE = (BM + BN) * F32_LDK;         // floats per LDS buffer
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave & 1, wn = wave >> 1;
  // tile walk: XCD-contiguous ids, groups of G32_GROUP_M M-tiles, M fastest inside a group
  const int id = xcd_remap((int)blockIdx.x, (int)gridDim.x);
  const int per_group = G32_GROUP_M * a.tiles_n;
  const int grp = id / per_group, in_grp = id - grp * per_group;
  const int gm = min(G32_GROUP_M, a.tiles_m - grp * G32_GROUP_M);
  const int tm = grp * G32_GROUP_M + in_grp % gm, tn = in_grp / gm;
  const int m0 = tm * BM, n0 = tn * BN;
  const int q = tid & 7, r0 = tid >> 3;

  const float* arow_g[AL];
  const float* brow_g[BL];
#pragma unroll
  for (int i = 0; i < AL; ++i) arow_g[i] = a.X + (size_t)min(m0 + r0 + 32 * i, a.M - 1) * a.ldx + 4 * q;
#pragma unroll
  for (int i = 0; i < BL; ++i) brow_g[i] = a.W + (size_t)min(n0 + r0 + 32 * i, a.N - 1) * a.ldw + 4 * q;

  f32x4_t ra[AL], rb[BL];
  auto fetch = [&](int kb) {
#pragma unroll
    for (int i = 0; i < AL; ++i) ra[i] = *(const f32x4_t*)(arow_g[i] + kb);
#pragma unroll
    for (int i = 0; i < BL; ++i) rb[i] = *(const f32x4_t*)(brow_g[i] + kb);
  };
  auto stash = [&](int buf) {
    float* s = smem + buf * STAGE;
#pragma unroll
    for (int i = 0; i < AL; ++i) *(f32x4_t*)(s + (r0 + 32 * i) * F32_LDK + 4 * q) = ra[i];
#pragma unroll
    for (int i = 0; i < BL; ++i) *(f32x4_t*)(s + (BM + r0 + 32 * i) * F32_LDK + 4 * q) = rb[i];
  };

  f32x16_t acc[RB][CB];
  f32_tile_zero(acc);

  const int arow = f32_tile_lane_offset(wm * RB * 32, lane);
  const int brow = f32_tile_lane_offset(BM + wn * CB * 32, lane);
  const int nk = a.K / F32_BK;
  fetch(0);
  stash(0);
  __syncthreads();
  for (int st = 0; st < nk; ++st) {
    const int cur = st & 1;
    if (st + 1 < nk) fetch((st + 1) * F32_BK);
    f32_tile_stage<RB, CB>(smem + cur * STAGE, arow, brow, acc);
    if (st + 1 < nk) stash(cur ^ 1);
    __syncthreads();
  }

  // epilogue: 32x32 C/D map -- column = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5); 32 lanes store 128
  // contiguous bytes of one row
#pragma unroll
  for (int j = 0; j < CB; ++j) {
    const int n = n0 + (wn * CB + j) * 32 + (lane & 31);
    if (n >= a.N) continue;
    const float b = a.bias ? a.bias[n] : 0.f;
#pragma unroll
    for (int i = 0; i < RB; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = m0 + (wm * RB + i) * 32 + f32_tile_row(r, lane);
        if (m >= a.M) continue;
        float v = acc[i][j][r] + b;
        if constexpr (EPI == G32_GELU) v = gelu_erf(v);
        if constexpr (EPI == G32_RESID) v += a.R[(size_t)(a.rmod > 0 ? m % a.rmod : m) * a.ldr + n];
        a.C[(size_t)m * a.ldc + n] = v;
      }
  }
}

template <int RB, int CB, int EPI>
int launch_gemm_f32(GemmF32Args g, hipStream_t s) {
  constexpr int BM = 2 * RB * 32, BN = 2 * CB * 32, LDS = gemm_f32_lds_bytes<RB, CB>();
  auto kern = gemm_f32_kernel<RB, CB, EPI>;
  static HmLdsOnce lds_once;
  if (const int rc = lds_once.ensure((const void*)kern, LDS, "hm_gemm_f32: cannot raise the dynamic LDS limit")) return rc;
  g.tiles_m = (g.M + BM - 1) / BM;
  g.tiles_n = (g.N + BN - 1) / BN;
  hipLaunchKernelGGL(kern, dim3((unsigned)(g.tiles_m * g.tiles_n)), dim3(256), LDS, s, g);
  return hm_check_launch("hm_gemm_f32");
}

// the tile changes which threads compute an output, never its arithmetic (see the numerics contract above)
template <int EPI>
int dispatch_gemm_f32(const GemmF32Args& g, hipStream_t s) {
  const long tiles = (long)((g.M + 127) / 128) * ((g.N + 127) / 128);
  if (tiles < hm_device_cu_count()) return launch_gemm_f32<1, 1, EPI>(g, s);   // 64 x 64: a few hands
  return launch_gemm_f32<2, 2, EPI>(g, s);                                      // 128 x 128
}

}  // namespace

extern "C" int hm_gemm_f32(const hm_gemm_args* a, void* stream_) {
  if (!a) return hm_set_error(HM_ERR_ARG, "hm_gemm_f32: null args");
  const hm_gemm_args& c = *a;
  if (c.dtype != HM_DTYPE_F32) return hm_set_error(HM_ERR_ARG, "hm_gemm_f32: dtype must be HM_DTYPE_F32");
  if (!c.X || !c.W || !c.C) return hm_set_error(HM_ERR_ARG, "hm_gemm_f32: null operand");
  if (c.M <= 0 || c.N <= 0 || c.K <= 0 || (long)c.M * c.N >= (1l << 40)) return hm_set_error(HM_ERR_ARG, "hm_gemm_f32: empty or oversized problem");
  if (c.K % F32_BK != 0) return hm_set_error(HM_ERR_ARG, "hm_gemm_f32: K must be a multiple of 32");
  if (c.ldx % 4 != 0 || c.ldw % 4 != 0 || c.ldx < c.K || c.ldw < c.K || c.ldc < c.N)
    return hm_set_error(HM_ERR_ARG, "hm_gemm_f32: ldx, ldw multiples of 4 and >= K, ldc >= N");
  if ((((uintptr_t)c.X | (uintptr_t)c.W) & 15) || (((uintptr_t)c.C | (uintptr_t)c.bias | (uintptr_t)c.resid) & 3))
    return hm_set_error(HM_ERR_ARG, "hm_gemm_f32: X / W 16-byte aligned, C / bias / resid 4-byte aligned");
  if (c.epilogue != HM_EPI_F32 && c.epilogue != HM_EPI_GELU && c.epilogue != HM_EPI_RESID_F32)
    return hm_set_error(HM_ERR_ARG, "hm_gemm_f32: epilogue is HM_EPI_F32, HM_EPI_GELU or HM_EPI_RESID_F32 (C is fp32 in all three)");
  if (c.k_split > 1 || c.ln_gamma || c.ln_xg || c.ln_stats || c.ln_colsum || (c.out_scale != 0.f && c.out_scale != 1.f))
    return hm_set_error(HM_ERR_ARG, "hm_gemm_f32: no split-K, no deferred LayerNorm, no output prescale on the fp32 route");
  if (c.epilogue == HM_EPI_RESID_F32 && (!c.resid || c.ldr < c.N || c.resid_mod < 0))
    return hm_set_error(HM_ERR_ARG, "hm_gemm_f32: HM_EPI_RESID_F32 needs resid with ldr >= N and resid_mod >= 0");
  if ((long)((c.M + 63) / 64) * ((c.N + 63) / 64) >= (1l << 31)) return hm_set_error(HM_ERR_ARG, "hm_gemm_f32: too many tiles");
  GemmF32Args g{};
  g.X = (const float*)c.X; g.W = (const float*)c.W; g.bias = c.bias; g.R = c.resid; g.C = (float*)c.C;
  g.M = c.M; g.N = c.N; g.K = c.K; g.ldx = c.ldx; g.ldw = c.ldw; g.ldc = c.ldc; g.ldr = c.ldr; g.rmod = c.resid_mod;
  hipStream_t s = (hipStream_t)stream_;
  HmProfScope prof(HM_K_GEMM, c.epilogue, c.M, c.N, c.K, s);
  if (c.epilogue == HM_EPI_GELU) return dispatch_gemm_f32<G32_GELU>(g, s);
  if (c.epilogue == HM_EPI_RESID_F32) return dispatch_gemm_f32<G32_RESID>(g, s);
  return dispatch_gemm_f32<G32_BIAS>(g, s);
}
