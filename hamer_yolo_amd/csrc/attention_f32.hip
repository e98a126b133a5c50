// hm_vit_attention_f32: Attention.forward's core (vit.py:115-123) in fp32 for the precise HaMeR route -- 192 tokens, heads of 80.
//   q = q * scale (fp32, as the reference scales q before the product, vit.py:116-117); S = q . k^T; P = softmax(S) with the row
//   maximum subtracted, expf, and the row sum taken in one fixed order; out = P . V, head-major [B * 192][heads * 80].
// Everything is fp32: both products run on v_mfma_f32_16x16x4_f32 (f32 in, f32 accumulate, a k-ordered fmaf chain), the
// softmax on the vector ALU with IEEE division.  No value depends on anything but its own (hand, head, query row): one hand
// alone gives the same bytes as that hand inside any batch.
//
// One workgroup (256 threads) per (hand, head, 64 query rows); Q, K and V of one (hand, head) are 3 x 61 KB and do not fit the
// LDS together, so K and V take turns in one buffer:
//   LDS: Qs [64][84] (scaled q), KVs [192][84] (K, later V), Ss [64][196] (scores, then probabilities)   = 133 KB
//   1. Q chunk and K -> LDS.                      2. wave w: S rows 16w .. 16w+15 against the 12 key blocks of 16 -> Ss.
//   3. V -> KVs; softmax: 4 adjacent lanes per row, lane j owns keys 4i + j; row sum = each lane's 48 terms in order, then
//      (l0 + l1) + (l2 + l3) over the lanes.   4. wave w: out rows 16w .. 16w+15 = P . V over 5 column blocks of 16.
// MFMA operand maps (16x16x4, f32): lane l holds A[l & 15][k = l >> 4] and B[k = l >> 4][l & 15]; within a group of 16 k every
// lane reads 4 consecutive k (one 16-byte LDS read), MFMA e of the group consumes element e, i.e. k-slot s of MFMA e is
// k = 16g + 4s + e on both operands (hm_linear_f32's order).  C/D: lane l holds D[4 (l >> 4) + r][l & 15].
// At 6 GFLOP per hand this is 2.4 % of the route's work: it is written for the fixed order, not for the last cycle.
#include <math.h>
#include "common.h"
#include "hamer_hip_internal.h"

namespace {

constexpr int AF_T = 192, AF_HD = 80, AF_QC = 64;      // tokens, head dim, query rows per workgroup
constexpr int AF_LDH = AF_HD + 4, AF_LDS_S = AF_T + 4;  // LDS row strides in floats (16-byte aligned rows)
constexpr int AF_LDS_BYTES = (AF_QC * AF_LDH + AF_T * AF_LDH + AF_QC * AF_LDS_S) * 4;

__global__ __launch_bounds__(256) void attention_f32_kernel(const float* __restrict__ qkv, float* __restrict__ out, int heads,
                                                            float scale) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* Qs = smem;
  float* KVs = Qs + AF_QC * AF_LDH;
  float* Ss = KVs + AF_T * AF_LDH;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int chunk = blockIdx.x % (AF_T / AF_QC), bh = blockIdx.x / (AF_T / AF_QC);
  const int h = bh % heads, b = bh / heads;
  const int D = heads * AF_HD, ld = 3 * D, q0 = chunk * AF_QC;
  const float* base = qkv + (size_t)b * AF_T * ld + h * AF_HD;

  // ---- 1. Q chunk (scaled) and K
#pragma unroll
  for (int i = 0; i < AF_QC * (AF_HD / 4) / 256; ++i) {
    const int idx = tid + 256 * i, row = idx / (AF_HD / 4), c4 = idx % (AF_HD / 4);
    f32x4_t v = *(const f32x4_t*)(base + (size_t)(q0 + row) * ld + 4 * c4);
    v[0] *= scale; v[1] *= scale; v[2] *= scale; v[3] *= scale;
    *(f32x4_t*)(Qs + row * AF_LDH + 4 * c4) = v;
  }
#pragma unroll
  for (int i = 0; i < AF_T * (AF_HD / 4) / 256; ++i) {
    const int idx = tid + 256 * i, row = idx / (AF_HD / 4), c4 = idx % (AF_HD / 4);
    *(f32x4_t*)(KVs + row * AF_LDH + 4 * c4) = *(const f32x4_t*)(base + D + (size_t)row * ld + 4 * c4);
  }
  __syncthreads();

  // ---- 2. scores
  const int li = lane & 15, ks = lane >> 4;
  {
    f32x4_t acc[AF_T / 16];
#pragma unroll
    for (int kb = 0; kb < AF_T / 16; ++kb) acc[kb] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    const float* qrow = Qs + (wave * 16 + li) * AF_LDH + 4 * ks;
    const float* krow = KVs + li * AF_LDH + 4 * ks;
#pragma unroll
    for (int g = 0; g < AF_HD / 16; ++g) {
      const f32x4_t av = *(const f32x4_t*)(qrow + 16 * g);
      f32x4_t bv[AF_T / 16];
#pragma unroll
      for (int kb = 0; kb < AF_T / 16; ++kb) bv[kb] = *(const f32x4_t*)(krow + kb * 16 * AF_LDH + 16 * g);
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int kb = 0; kb < AF_T / 16; ++kb) acc[kb] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[e], bv[kb][e], acc[kb], 0, 0, 0);
    }
#pragma unroll
    for (int kb = 0; kb < AF_T / 16; ++kb)
#pragma unroll
      for (int r = 0; r < 4; ++r) Ss[(wave * 16 + 4 * ks + r) * AF_LDS_S + kb * 16 + li] = acc[kb][r];
  }
  __syncthreads();      // every wave is done with K; the scores are visible

  // ---- 3. V into the K buffer, softmax in place
#pragma unroll
  for (int i = 0; i < AF_T * (AF_HD / 4) / 256; ++i) {
    const int idx = tid + 256 * i, row = idx / (AF_HD / 4), c4 = idx % (AF_HD / 4);
    *(f32x4_t*)(KVs + row * AF_LDH + 4 * c4) = *(const f32x4_t*)(base + 2 * D + (size_t)row * ld + 4 * c4);
  }
  {
    float* srow = Ss + (tid >> 2) * AF_LDS_S + (tid & 3);
    float s[AF_T / 4];
    float mx = -INFINITY;
#pragma unroll
    for (int i = 0; i < AF_T / 4; ++i) { s[i] = srow[4 * i]; mx = fmaxf(mx, s[i]); }
    mx = fmaxf(mx, __shfl_xor(mx, 1, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 2, 64));
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < AF_T / 4; ++i) { s[i] = expf(s[i] - mx); sum += s[i]; }
    sum = sum + __shfl_xor(sum, 1, 64);          // (l0 + l1), (l2 + l3): the same value on both lanes of a pair
    sum = sum + __shfl_xor(sum, 2, 64);          // (l0 + l1) + (l2 + l3) on all four
#pragma unroll
    for (int i = 0; i < AF_T / 4; ++i) srow[4 * i] = s[i] / sum;
  }
  __syncthreads();

  // ---- 4. out = P . V
  {
    f32x4_t acc[AF_HD / 16];
#pragma unroll
    for (int cb = 0; cb < AF_HD / 16; ++cb) acc[cb] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    const float* prow = Ss + (wave * 16 + li) * AF_LDS_S + 4 * ks;
    const float* vcol = KVs + (4 * ks) * AF_LDH + li;
#pragma unroll 2
    for (int g = 0; g < AF_T / 16; ++g) {
      const f32x4_t av = *(const f32x4_t*)(prow + 16 * g);
      f32x4_t bv[AF_HD / 16];
#pragma unroll
      for (int cb = 0; cb < AF_HD / 16; ++cb)
#pragma unroll
        for (int e = 0; e < 4; ++e) bv[cb][e] = vcol[(16 * g + e) * AF_LDH + 16 * cb];
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int cb = 0; cb < AF_HD / 16; ++cb) acc[cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[e], bv[cb][e], acc[cb], 0, 0, 0);
    }
    float* orow = out + ((size_t)b * AF_T + q0 + wave * 16 + 4 * ks) * D + h * AF_HD + li;
#pragma unroll
    for (int cb = 0; cb < AF_HD / 16; ++cb)
#pragma unroll
      for (int r = 0; r < 4; ++r) orow[(size_t)r * D + 16 * cb] = acc[cb][r];
  }
}

}  // namespace

extern "C" int hm_vit_attention_f32(const float* qkv, float* out, int B, int tokens, int heads, int head_dim, float scale,
                                    void* stream_) {
  if (!qkv || !out || B <= 0 || heads <= 0) return hm_set_error(HM_ERR_ARG, "hm_vit_attention_f32: bad arguments");
  if (tokens != AF_T || head_dim != AF_HD) return hm_set_error(HM_ERR_ARG, "hm_vit_attention_f32: 192 tokens and head_dim 80 only");
  if (((uintptr_t)qkv | (uintptr_t)out) & 15) return hm_set_error(HM_ERR_ARG, "hm_vit_attention_f32: pointers must be 16-byte aligned");
  if ((long)B * heads * (AF_T / AF_QC) >= (1l << 31)) return hm_set_error(HM_ERR_ARG, "hm_vit_attention_f32: batch too large");
  static HmLdsOnce lds_once;
  if (const int rc = lds_once.ensure((const void*)attention_f32_kernel, AF_LDS_BYTES, "hm_vit_attention_f32: cannot raise the dynamic LDS limit")) return rc;
  hipStream_t s = (hipStream_t)stream_;
  HmProfScope prof(HM_K_ATTENTION, 0, B, tokens, heads, s);
  hipLaunchKernelGGL(attention_f32_kernel, dim3((unsigned)(B * heads * (AF_T / AF_QC))), dim3(256), AF_LDS_BYTES, s, qkv, out, heads, scale);
  return hm_check_launch("hm_vit_attention_f32");
}
