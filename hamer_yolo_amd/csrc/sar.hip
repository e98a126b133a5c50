// SAR hand-mesh head of the RootNet checkpoint (rootnet/Model_RGB.py:76-177, SARhead :198-222) and the post-processing of
// EstimateRGB.run (:428-480, :500-570), for all B hands of a call at once.
//
// Activations are node-major across the batch, [778 nodes][B hands][C], so that
//   * GraphConv's L . X (L = A / (rowsum(A) + 1e-5), one dense 778 x 778 matrix per layer) is ONE GEMM with M = 778,
//     K = 778, N = B * C, its activation operand read row-major [K][N] and transposed on the LDS read
//     (ds_read_b64_tr_b16);
//   * GraphConv's fc is a plain NT GEMM over the 778 * B rows.
// The SAIGB 1x1 convolution is an NT GEMM with the 6224 output channels as M and the B * 64 feature positions as N; its
// epilogue adds the bias, applies LeakyReLU(0.1), moves channel c / position p of hand b to node c / 8, column
// (c % 8) * 64 + p (the reference's .view(-1, 778, 512) of NCHW) and writes the template columns and the zero K padding.
// All GEMMs: f16 operands, fp32 accumulation, 128 x 128 tiles of four 64 x 64 waves, one k-ordered sum per output (no
// split-K): a hand's numbers do not depend on the batch it travels in.
#include <math.h>
#include "common.h"
#include "hamer_hip_internal.h"

namespace {

constexpr int NV = 778, NJ = 21, NT = NV + NJ, CELLS = 1024;
constexpr int KG = 544;          // SAIGB row: 512 features + 3 template + 29 zeros (K of the first fc, a multiple of 32)
constexpr int BM = 128, BN = 128, BK = 32;
constexpr int AST = 40;          // LDS row stride (elements) of the [128][32] A / NT-B images: 80 B
constexpr int XST = 136;         // LDS row stride (elements) of the [32][128] NN-B image: 272 B, 8-byte aligned rows

enum { G_SAIGB = 0, G_MIX = 1, G_FC_LEAKY = 2, G_FC_F32 = 3 };

struct GemmP {
  const _Float16* A;     // [M][lda], K contiguous (zero padded to K)
  const _Float16* B;     // NT: [N][ldb] K contiguous;  MIX: [kb_rows][ldb] N contiguous
  void* C;
  const float* bias;     // SAIGB: [M];  FC: [N]
  const float* tmpl;     // SAIGB: [778][3]
  int M, N, K, lda, ldb, ldc, kb_rows, hands;
};

__device__ __forceinline__ float leaky(float x) { return x > 0.f ? x : 0.1f * x; }

template <class V4> __device__ __forceinline__ V4 lds_read_tr4(const void* p) {
  typedef __attribute__((ext_vector_type(4))) short s16x4;
  const s16x4 v = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)p);
  return __builtin_bit_cast(V4, v);
}

template <int MODE>
__global__ __launch_bounds__(256) void sar_gemm_kernel(GemmP P) {
  constexpr bool NN = MODE == G_MIX;
  __shared__ __attribute__((aligned(16))) _Float16 As[BM * AST];
  __shared__ __attribute__((aligned(16))) _Float16 Bs[NN ? BK * XST : BN * AST];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1, g = lane >> 4, li = lane & 15;
  const int m0 = blockIdx.y * BM, n0 = blockIdx.x * BN;

  f16x8_t ra[2], rb[2];
  auto load = [&](int k0) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int c = tid + 256 * i;
      const int r = min(m0 + (c >> 2), P.M - 1);          // rows past M read row M-1: finite, never stored
      ra[i] = *(const f16x8_t*)(P.A + (size_t)r * P.lda + k0 + (c & 3) * 8);
      if constexpr (NN) {
        const int kr = min(k0 + (c >> 4), P.kb_rows - 1);  // k rows past the last node meet zero columns of L
        const int cn = min(n0 + (c & 15) * 8, P.N - 8);
        rb[i] = *(const f16x8_t*)(P.B + (size_t)kr * P.ldb + cn);
      } else {
        const int rn = min(n0 + (c >> 2), P.N - 1);
        rb[i] = *(const f16x8_t*)(P.B + (size_t)rn * P.ldb + k0 + (c & 3) * 8);
      }
    }
  };
  auto stash = [&]() {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int c = tid + 256 * i;
      *(f16x8_t*)(As + (c >> 2) * AST + (c & 3) * 8) = ra[i];
      if constexpr (NN) *(f16x8_t*)(Bs + (c >> 4) * XST + (c & 15) * 8) = rb[i];
      else *(f16x8_t*)(Bs + (c >> 2) * AST + (c & 3) * 8) = rb[i];
    }
  };

  f32x4_t acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  load(0);
  for (int k0 = 0; k0 < P.K; k0 += BK) {
    stash();
    __syncthreads();
    if (k0 + BK < P.K) load(k0 + BK);
    f16x8_t af[4], bf[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) af[i] = *(const f16x8_t*)(As + (wm * 64 + i * 16 + li) * AST + 8 * g);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if constexpr (NN) {
        // lane 4q+p of each 16-lane group addresses row 8g+q (then 8g+4+q), columns 4p..4p+3 of the 16-column block;
        // it receives column li of those 4 rows: k = 8g .. 8g+7 of column li, the B-operand map
        const _Float16* blk = Bs + (8 * g + (li >> 2)) * XST + wn * 64 + j * 16 + 4 * (li & 3);
        const f16x4_t lo = lds_read_tr4<f16x4_t>(blk), hi = lds_read_tr4<f16x4_t>(blk + 4 * XST);
#pragma unroll
        for (int e = 0; e < 4; ++e) { bf[j][e] = lo[e]; bf[j][4 + e] = hi[e]; }
      } else {
        bf[j] = *(const f16x8_t*)(Bs + (wn * 64 + j * 16 + li) * AST + 8 * g);
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = TF16::mfma(af[i], bf[j], acc[i][j]);
    __syncthreads();
  }

  // lane holds D[row 4g + r][col li] of each 16 x 16 tile
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int n = n0 + wn * 64 + j * 16 + li;
      if (n >= P.N) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = m0 + wm * 64 + i * 16 + 4 * g + r;
        if (m >= P.M) continue;
        float v = acc[i][j][r];
        if constexpr (MODE == G_SAIGB) {
          v = leaky(v + P.bias[m]);
          const int node = m >> 3, b = n >> 6, p = n & 63;
          _Float16* row = (_Float16*)P.C + ((size_t)node * P.hands + b) * KG;
          row[(m & 7) * 64 + p] = (_Float16)v;
          if ((m & 7) == 0 && p == 0)
            for (int t = 0; t < KG - 512; ++t) row[512 + t] = t < 3 ? (_Float16)P.tmpl[node * 3 + t] : (_Float16)0.f;
        } else if constexpr (MODE == G_MIX) {
          ((_Float16*)P.C)[(size_t)m * P.ldc + n] = (_Float16)v;
        } else if constexpr (MODE == G_FC_LEAKY) {
          ((_Float16*)P.C)[(size_t)m * P.ldc + n] = (_Float16)leaky(v + P.bias[n]);
        } else {
          ((float*)P.C)[(size_t)m * P.ldc + n] = v + P.bias[n];
        }
      }
    }
}

template <int MODE> int launch_gemm(const GemmP& p, hipStream_t s, const char* what) {
  HmProfScope prof(HM_K_GEMM, 100 + MODE, p.M, p.N, p.K, s);
  dim3 grid((p.N + BN - 1) / BN, (p.M + BM - 1) / BM);
  hipLaunchKernelGGL(sar_gemm_kernel<MODE>, grid, dim3(256), 0, s, p);
  return hm_check_launch(what);
}

// mesh2pose_hm / mesh2pose_dm (nn.Linear(778, 21) over the vertex axis, :168-169): rows 778 .. 798 of a branch's
// [799][B*1024] fp32 logits from its rows 0 .. 777.  One thread per (hand, cell) column, the 778 vertices in order.
__global__ __launch_bounds__(256) void sar_mesh2pose_kernel(float* __restrict__ lxy, float* __restrict__ lz, const float* __restrict__ w_xy,
                                                            const float* __restrict__ b_xy, const float* __restrict__ w_z,
                                                            const float* __restrict__ b_z, int cols) {
  float* L = blockIdx.y ? lz : lxy;
  const float* W = blockIdx.y ? w_z : w_xy;        // [21][778]
  const float* bias = blockIdx.y ? b_z : b_xy;
  const int col = blockIdx.x * 256 + threadIdx.x;
  if (col >= cols) return;
  float acc[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) acc[j] = 0.f;
  for (int v = 0; v < NV; ++v) {
    const float x = L[(size_t)v * cols + col];
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[j] = fmaf(W[j * NV + v], x, acc[j]);
  }
#pragma unroll
  for (int j = 0; j < NJ; ++j) L[(size_t)(NV + j) * cols + col] = acc[j] + bias[j];
}

// SoftHeatmap (:76-99) and GBBMR's coordinate sums (:170-176): one wave per (hand, node); 16 cells per lane.
__global__ __launch_bounds__(256) void sar_softargmax_kernel(const float* __restrict__ lxy, const float* __restrict__ lz,
                                                             const float* __restrict__ beta, const float* __restrict__ wx,
                                                             const float* __restrict__ wy, float* __restrict__ coords, int B) {
  const int lane = threadIdx.x & 63;
  const int item = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (item >= B * NT) return;                       // (wave-uniform)
  const int b = item / NT, n = item % NT;
  const size_t row = ((size_t)n * B + b) * CELLS;
  const float bt = beta[n];
  float s[16], z[16];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const f32x4_t a = *(const f32x4_t*)(lxy + row + i * 256 + lane * 4);
    const f32x4_t c = *(const f32x4_t*)(lz + row + i * 256 + lane * 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) { s[4 * i + e] = a[e] * bt; z[4 * i + e] = c[e]; }
  }
  float mx = s[0];
#pragma unroll
  for (int i = 1; i < 16; ++i) mx = fmaxf(mx, s[i]);
  mx = wave_max(mx);
  float sum = 0.f;
#pragma unroll
  for (int i = 0; i < 16; ++i) { s[i] = expf(s[i] - mx); sum += s[i]; }
  sum = wave_sum(sum);
  float px = 0.f, py = 0.f, pz = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int c = i * 256 + lane * 4 + e;
      const float p = s[4 * i + e] / sum;
      px = fmaf(p, wx[c], px);
      py = fmaf(p, wy[c], py);
      pz = fmaf(p, z[4 * i + e], pz);
    }
  px = wave_sum(px); py = wave_sum(py); pz = wave_sum(pz);
  if (lane == 0) {
    float* o = coords + ((size_t)b * NT + n) * 3;
    o[0] = px / 16.f - 1.f;
    o[1] = py / 16.f - 1.f;
    o[2] = pz;
  }
}

// grid_sample(depth[None, None], grid, bilinear, zeros, align_corners=False) at one normalised point
__device__ float sample_depth(const float* d, int W, int H, float gx, float gy) {
  const float ix = ((gx + 1.f) * W - 1.f) * 0.5f, iy = ((gy + 1.f) * H - 1.f) * 0.5f;
  const float fx0 = floorf(ix), fy0 = floorf(iy);
  const int x0 = (int)fx0, y0 = (int)fy0;
  const float tx = ix - fx0, ty = iy - fy0;
  float acc = 0.f;
#pragma unroll
  for (int dy = 0; dy < 2; ++dy)
#pragma unroll
    for (int dx = 0; dx < 2; ++dx) {
      const int x = x0 + dx, y = y0 + dy;
      const float w = (dx ? tx : 1.f - tx) * (dy ? ty : 1.f - ty);
      if (x >= 0 && x < W && y >= 0 && y < H) acc += w * d[(size_t)y * W + x];
    }
  return acc;
}

// post_processing (:428-480) plus the root depth of run (:533-551): one thread per (hand, node)
__global__ __launch_bounds__(256) void sar_post_kernel(const float* __restrict__ coords, const hm_sar_hand* __restrict__ hands,
                                                       const float* __restrict__ root, const float* __restrict__ depth,
                                                       float* __restrict__ uvd, float* __restrict__ xyz, int B, int P) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= B * NT) return;
  const int b = i / NT;
  const hm_sar_hand h = hands[b];
  const float* c = coords + (size_t)i * 3;
  const float* t = h.bb2img;
  float r = root ? root[b] : 0.f;
  if (h.depth_offset >= 0 && depth) {              // convert2origin_pixel of row 778 (NOT un-flipped), then grid_sample
    const float* cr = coords + ((size_t)b * NT + NV) * 3;
    const float u = __fmul_rn(__fadd_rn(cr[0], 0.5f), (float)P), v = __fmul_rn(__fadd_rn(cr[1], 0.5f), (float)P);
    const float fu = __fadd_rn(__fadd_rn(__fmul_rn(t[0], u), __fmul_rn(t[1], v)), t[2]);
    const float fv = __fadd_rn(__fadd_rn(__fmul_rn(t[3], u), __fmul_rn(t[4], v)), t[5]);
    r = sample_depth(depth + h.depth_offset, h.depth_w, h.depth_h, fu / (float)(h.img_w / 2) - 1.f, fv / (float)(h.img_h / 2) - 1.f);
  }
  const float z = __fadd_rn(__fmul_rn(c[2], h.depth_box), r);
  const float u = __fmul_rn(__fadd_rn(c[0], 0.5f), (float)P), v = __fmul_rn(__fadd_rn(c[1], 0.5f), (float)P);
  float fu = __fadd_rn(__fadd_rn(__fmul_rn(t[0], u), __fmul_rn(t[1], v)), t[2]);
  const float fv = __fadd_rn(__fadd_rn(__fmul_rn(t[3], u), __fmul_rn(t[4], v)), t[5]);
  if (h.flip) fu = __fadd_rn(__fsub_rn((float)h.img_w, fu), -1.f);
  float* o = uvd + (size_t)i * 3;
  o[0] = fu; o[1] = fv; o[2] = z;
  float* q = xyz + (size_t)i * 3;                  // uvd2xyz (preprocessing.py:11-17), evaluated in double as numpy does with K
  q[0] = (float)(((double)fu - h.fu) * (double)z / h.fx);
  q[1] = (float)(((double)fv - h.fv) * (double)z / h.fy);
  q[2] = z;
}

}  // namespace

static int saigb_launch(const void* feat, const void* w, const float* bias, const float* tmpl, void* g, int B, int channels, void* stream) {
  GemmP p{(const _Float16*)w, (const _Float16*)feat, g, bias, tmpl, 8 * NV, B * 64, channels, channels, channels, 0, 0, B};
  return launch_gemm<G_SAIGB>(p, (hipStream_t)stream, "hm_sar_saigb");
}

// SAIGB on a backbone of `channels` feature channels (512: ResNet-34, 1024: ConvNeXt-base).  Only the K of the 1 x 1
// convolution changes: its 6224 output channels, and so the [778][B][544] graph, are the same.
extern "C" int hm_sar_saigb_ch(const void* feat, const void* w, const float* bias, const float* tmpl, void* g, int B, int channels,
                               void* stream) {
  if (!feat || !w || !bias || !tmpl || !g || B <= 0) return hm_set_error(HM_ERR_ARG, "hm_sar_saigb_ch: bad arguments");
  if (channels != 512 && channels != 1024) return hm_set_error(HM_ERR_ARG, "hm_sar_saigb_ch: channels must be 512 or 1024");
  if (((uintptr_t)feat | (uintptr_t)w) & 15) return hm_set_error(HM_ERR_ARG, "hm_sar_saigb_ch: feat and w must be 16-byte aligned");
  return saigb_launch(feat, w, bias, tmpl, g, B, channels, stream);
}

extern "C" int hm_sar_saigb(const void* feat, const void* w, const float* bias, const float* tmpl, void* g, int B, void* stream) {
  if (!feat || !w || !bias || !tmpl || !g || B <= 0) return hm_set_error(HM_ERR_ARG, "hm_sar_saigb: bad arguments");
  return saigb_launch(feat, w, bias, tmpl, g, B, 512, stream);
}

extern "C" int hm_sar_graph_mix(const void* lap, int ldl, const void* x, int N, void* y, void* stream) {
  if (!lap || !x || !y || N <= 0 || N % 8 != 0 || ldl < NV || ldl % BK != 0)
    return hm_set_error(HM_ERR_ARG, "hm_sar_graph_mix: bad arguments (N % 8 == 0, ldl >= 778, ldl % 32 == 0)");
  GemmP p{(const _Float16*)lap, (const _Float16*)x, y, nullptr, nullptr, NV, N, ldl, ldl, N, N, NV, 0};
  return launch_gemm<G_MIX>(p, (hipStream_t)stream, "hm_sar_graph_mix");
}

extern "C" int hm_sar_linear(const void* x, int M, int K, const void* w, const float* bias, void* y, int N, int out_f32, void* stream) {
  if (!x || !w || !bias || !y || M <= 0 || N <= 0 || K <= 0 || K % BK != 0)
    return hm_set_error(HM_ERR_ARG, "hm_sar_linear: bad arguments (K % 32 == 0)");
  GemmP p{(const _Float16*)x, (const _Float16*)w, y, bias, nullptr, M, N, K, K, K, N, 0, 0};
  return out_f32 ? launch_gemm<G_FC_F32>(p, (hipStream_t)stream, "hm_sar_linear")
                 : launch_gemm<G_FC_LEAKY>(p, (hipStream_t)stream, "hm_sar_linear");
}

extern "C" int hm_sar_softargmax(float* logits_xy, float* logits_z, const float* m2p_w_xy, const float* m2p_b_xy,
                                 const float* m2p_w_z, const float* m2p_b_z, const float* beta, const float* wx, const float* wy,
                                 float* coords, int B, void* stream) {
  if (!logits_xy || !logits_z || !m2p_w_xy || !m2p_b_xy || !m2p_w_z || !m2p_b_z || !beta || !wx || !wy || !coords || B <= 0)
    return hm_set_error(HM_ERR_ARG, "hm_sar_softargmax: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  const int cols = B * CELLS;
  {
    HmProfScope prof(HM_K_OTHER, 110, NJ, cols, NV, s);
    hipLaunchKernelGGL(sar_mesh2pose_kernel, dim3((cols + 255) / 256, 2), dim3(256), 0, s, logits_xy, logits_z, m2p_w_xy, m2p_b_xy,
                       m2p_w_z, m2p_b_z, cols);
    if (int rc = hm_check_launch("hm_sar_softargmax (mesh2pose)")) return rc;
  }
  HmProfScope prof(HM_K_OTHER, 111, B * NT, CELLS, 0, s);
  hipLaunchKernelGGL(sar_softargmax_kernel, dim3((B * NT + 3) / 4), dim3(256), 0, s, logits_xy, logits_z, beta, wx, wy, coords, B);
  return hm_check_launch("hm_sar_softargmax");
}

extern "C" int hm_sar_postprocess(const float* coords, const hm_sar_hand* hands, const float* root, const float* depth, float* uvd,
                                  float* xyz, int B, int P, void* stream) {
  if (!coords || !hands || !uvd || !xyz || B <= 0 || P <= 0) return hm_set_error(HM_ERR_ARG, "hm_sar_postprocess: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  HmProfScope prof(HM_K_OTHER, 112, B * NT, 0, 0, s);
  hipLaunchKernelGGL(sar_post_kernel, dim3((B * NT + 255) / 256), dim3(256), 0, s, coords, hands, root, depth, uvd, xyz, B, P);
  return hm_check_launch("hm_sar_postprocess");
}
