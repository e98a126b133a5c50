// The staged fp32 tile loop's MFMA side, shared by conv_f32.hip (implicit GEMM) and gemm_f32.hip (nn.Linear): both stage
// K in steps of F32_BK floats through an LDS tile of rows [A rows | B rows] with row stride F32_LDK, and both consume a stage
// in the same K order -- so a 1x1 convolution and a GEMM of the same operands sum in one order and give the same bytes.
//   v_mfma_f32_32x32x2_f32: lane l holds A[l & 31][k-slot l >> 5] and B[k-slot l >> 5][l & 31]; within a group g of 8 k, lanes
//   0-31 (k-slot 0) hold k = 8g + e and lanes 32-63 (k-slot 1) hold k = 8g + 4 + e, e = 0..3 the MFMA's index in the group:
//   one 16-byte LDS read per operand and group.  A wave owns RB x CB blocks of 32x32, each its own accumulator.
#pragma once
#include "common.h"

typedef __attribute__((ext_vector_type(16))) float f32x16_t;

constexpr int F32_BK = 32;             // K per stage
constexpr int F32_LDK = F32_BK + 4;    // LDS row stride in floats: 16-byte aligned rows that start in different banks

template <int RB, int CB>
__device__ __forceinline__ void f32_tile_zero(f32x16_t (&acc)[RB][CB]) {
#pragma unroll
  for (int i = 0; i < RB; ++i)
#pragma unroll
    for (int j = 0; j < CB; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
}

// a lane's offset into the LDS tile for the operand block that starts at tile row `row0`
__device__ __forceinline__ int f32_tile_lane_offset(int row0, int lane) { return (row0 + (lane & 31)) * F32_LDK + 4 * (lane >> 5); }

// one stage: acc[i][j] += A block i . B block j^T over the stage's F32_BK k, in k order
template <int RB, int CB>
__device__ __forceinline__ void f32_tile_stage(const float* s, int arow, int brow, f32x16_t (&acc)[RB][CB]) {
#pragma unroll
  for (int g = 0; g < F32_BK / 8; ++g) {
    f32x4_t av[RB], bv[CB];
#pragma unroll
    for (int i = 0; i < RB; ++i) av[i] = *(const f32x4_t*)(s + arow + i * 32 * F32_LDK + 8 * g);
#pragma unroll
    for (int j = 0; j < CB; ++j) bv[j] = *(const f32x4_t*)(s + brow + j * 32 * F32_LDK + 8 * g);
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int i = 0; i < RB; ++i)
#pragma unroll
        for (int j = 0; j < CB; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i][e], bv[j][e], acc[i][j], 0, 0, 0);
  }
}

// C/D map of the 32x32 block: column = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5), r the accumulator register
__device__ __forceinline__ int f32_tile_row(int r, int lane) { return (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5); }
