// The memory-bound kernels of the ConvNeXt-base SAR backbone (rootnet/convnext.py:15-50 Block, :66-114 ConvNeXt): everything
// of the network that is not a GEMM.  The residual stream is fp32 NHWC, [B][H][W][C]; each kernel reads it once and writes the
// 16-bit X operand of the hm_gemm launch that follows.  All arithmetic in fp32, one rounding at the store.
//   hm_dwconv7_ln    Block.dwconv (7 x 7 depthwise, padding 3, bias) + Block.norm (LayerNorm over C)       one per block
//   hm_ln_patchify2  downsample_layers[i][0] (LayerNorm over C) + the im2col of the 2 x 2 stride-2 convolution behind it
//   hm_stem4_im2col  the im2col of the 4 x 4 stride-4 stem convolution on the crop kernel's fp32 planes
// Every output pixel is computed by one fixed sequence of operations that depends on C alone: a hand's bytes do not depend on
// the batch it travels in or on its position.
#include "common.h"
#include "hamer_hip_internal.h"

namespace {

template <class E> struct Vec4Of;
template <> struct Vec4Of<__bf16> { using type = bf16x4_t; };
template <> struct Vec4Of<_Float16> { using type = f16x4_t; };

template <class E> __device__ __forceinline__ void store4h(E* p, f32x4_t v) {
  typename Vec4Of<E>::type o;
  o[0] = (E)v[0]; o[1] = (E)v[1]; o[2] = (E)v[2]; o[3] = (E)v[3];
  *(typename Vec4Of<E>::type*)p = o;
}

// ---------------------------------------------------------------------------------------------------------------
// Depthwise 7 x 7 + LayerNorm.  A thread owns 4 consecutive channels (16-byte loads; consecutive lanes, consecutive channels)
// and a run of RUN output pixels along x: per input row it loads the RUN + 6 pixels under the window once and slides the seven
// taps over them in registers (7 * (RUN + 6) / RUN = 12.25 pixel loads per output instead of 49, and the 49 weight
// loads serve RUN outputs; the kernel is bound by these L1 / L2 loads, not by HBM: RUN = 8 measured 1.1 - 1.3x faster than
// RUN = 4; DESIGN section 9.2 has the achieved GB/s per stage).  The CG = C / 4 threads of a pixel then reduce through LDS: partial sums are stored per thread, T = 256 / (PG * RUN) threads per pixel add CG / T of them each in
// a fixed order and finish with xor shuffles; mean first, then the squared deviations (the two-pass form of hm_layernorm).
// A workgroup of 256 threads is PG pixel groups x CG channel groups (PG the largest power of two with PG * CG <= 256) and
// covers PG * RUN pixels of one image row; the rows above and below are re-read by the neighbouring workgroups from L2.
constexpr int RUN = 8;

// red: [PG * RUN][CG] floats; v[r]: this thread's partial of pixel (pg, r).  Returns the pixel totals, the same bits in every
// thread of the pixel.  tot: [PG * RUN] floats.
__device__ __forceinline__ void pixel_reduce(float (&v)[RUN], float* red, float* tot, int pg, int cg, int CG, int PG, bool active) {
  const int tid = threadIdx.x;
  if (active) {
#pragma unroll
    for (int r = 0; r < RUN; ++r) red[(pg * RUN + r) * CG + cg] = v[r];
  }
  __syncthreads();
  const int npix = PG * RUN, T = 256 / npix;           // T is a power of two, 1 .. 256 / RUN <= 64
  const int pix = tid / T, t = tid % T;
  float s = 0.f;
  for (int i = t; i < CG; i += T) s += red[pix * CG + i];
  for (int o = T >> 1; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if (t == 0) tot[pix] = s;
  __syncthreads();
  if (active) {
#pragma unroll
    for (int r = 0; r < RUN; ++r) v[r] = tot[pg * RUN + r];
  }
}

template <class E>
__global__ __launch_bounds__(256) void dwconv7_ln_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                         const float* __restrict__ bias, const float* __restrict__ gamma,
                                                         const float* __restrict__ beta, E* __restrict__ out, int H, int W, int C,
                                                         int PG, int xblocks, float eps) {
  __shared__ float red[256 * RUN];
  __shared__ float tot[256];
  const int CG = C >> 2;
  const int tid = threadIdx.x;
  const int pg = tid / CG, cg = tid % CG;
  const bool active = pg < PG;
  int bid = blockIdx.x;
  const int xb = bid % xblocks; bid /= xblocks;
  const int y = bid % H, b = bid / H;
  const int x0 = (xb * PG + pg) * RUN;
  const int c = cg * 4;

  f32x4_t acc[RUN];
  if (active) {
    const f32x4_t bv = *(const f32x4_t*)(bias + c);
#pragma unroll
    for (int r = 0; r < RUN; ++r) acc[r] = bv;
    if (x0 < W) {
      for (int ky = 0; ky < 7; ++ky) {
        const int yy = y + ky - 3;
        if (yy < 0 || yy >= H) continue;                 // (a zero row adds nothing: the sum keeps its order)
        const float* row = x + ((size_t)(b * H + yy) * W) * C + c;
        f32x4_t in[RUN + 6], wk[7];
#pragma unroll
        for (int i = 0; i < RUN + 6; ++i) {
          const int xx = x0 + i - 3;
          in[i] = (xx >= 0 && xx < W) ? *(const f32x4_t*)(row + (size_t)xx * C) : f32x4_t{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int kx = 0; kx < 7; ++kx) wk[kx] = *(const f32x4_t*)(w + (size_t)(ky * 7 + kx) * C + c);
#pragma unroll
        for (int r = 0; r < RUN; ++r)
#pragma unroll
          for (int kx = 0; kx < 7; ++kx)
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[r][e] = fmaf(wk[kx][e], in[r + kx][e], acc[r][e]);
      }
    }
  }
  float v[RUN];
#pragma unroll
  for (int r = 0; r < RUN; ++r) v[r] = active ? (acc[r][0] + acc[r][1]) + (acc[r][2] + acc[r][3]) : 0.f;
  pixel_reduce(v, red, tot, pg, cg, CG, PG, active);
  float mean[RUN];
#pragma unroll
  for (int r = 0; r < RUN; ++r) {
    mean[r] = v[r] / (float)C;
    if (active) {
      const f32x4_t d = acc[r] - mean[r];
      v[r] = (d[0] * d[0] + d[1] * d[1]) + (d[2] * d[2] + d[3] * d[3]);
    }
  }
  pixel_reduce(v, red, tot, pg, cg, CG, PG, active);
  if (!active) return;
  const f32x4_t gv = *(const f32x4_t*)(gamma + c), be = *(const f32x4_t*)(beta + c);
#pragma unroll
  for (int r = 0; r < RUN; ++r) {
    const int xo = x0 + r;
    if (xo >= W) break;
    const float rstd = 1.0f / sqrtf(v[r] / (float)C + eps);
    store4h<E>(out + ((size_t)(b * H + y) * W + xo) * C + c, (acc[r] - mean[r]) * rstd * gv + be);
  }
}

// ---------------------------------------------------------------------------------------------------------------
// LayerNorm over C + 2 x 2 patchify: one wave per input pixel, the pixel in registers (hm_layernorm's two-pass statistics),
// written into the (ky, kx) quarter of its patch's row: out [B * H/2 * W/2][4C], column (ky * 2 + kx) * C + c.
template <class E, int MAXJ>
__global__ __launch_bounds__(256) void ln_patchify2_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                           const float* __restrict__ beta, E* __restrict__ out, int M, int H, int W,
                                                           int C, float eps) {
  const int lane = threadIdx.x & 63;
  const int pix = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (pix >= M) return;                                  // (wave-uniform)
  const float* xr = x + (size_t)pix * C;
  f32x4_t v[MAXJ];
#pragma unroll
  for (int j = 0; j < MAXJ; ++j) {
    const int i = lane * 4 + j * 256;
    v[j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    if (i < C) v[j] = *(const f32x4_t*)(xr + i);
  }
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < MAXJ; ++j) s += (v[j][0] + v[j][1]) + (v[j][2] + v[j][3]);
  const float mean = wave_sum(s) / (float)C;
  float q = 0.f;
#pragma unroll
  for (int j = 0; j < MAXJ; ++j) {
    const int i = lane * 4 + j * 256;
    if (i < C) {
      const f32x4_t d = v[j] - mean;
      q += (d[0] * d[0] + d[1] * d[1]) + (d[2] * d[2] + d[3] * d[3]);
    }
  }
  const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)C + eps);
  const int xx = pix % W, yy = (pix / W) % H, b = pix / (W * H);
  const size_t prow = ((size_t)b * (H >> 1) + (yy >> 1)) * (W >> 1) + (xx >> 1);
  E* orow = out + prow * 4 * C + (size_t)((yy & 1) * 2 + (xx & 1)) * C;
#pragma unroll
  for (int j = 0; j < MAXJ; ++j) {
    const int i = lane * 4 + j * 256;
    if (i < C) store4h<E>(orow + i, (v[j] - mean) * rstd * *(const f32x4_t*)(gamma + i) + *(const f32x4_t*)(beta + i));
  }
}

// ---------------------------------------------------------------------------------------------------------------
// Stem im2col: img [B][3][H][W] fp32 planes -> rows [B * H/4 * W/4][64] 16-bit, column c * 16 + ky * 4 + kx (the (c, ky, kx)
// order of Conv2d's weight) for the 48 values, columns 48 .. 63 zero (hm_gemm takes K in multiples of 64).  16 threads per
// patch, 8 bytes each: thread t < 12 moves the four kx of (c, ky) = (t / 4, t % 4), threads 12 .. 15 write the zeros.
template <class E>
__global__ __launch_bounds__(256) void stem4_im2col_kernel(const float* __restrict__ img, E* __restrict__ out, size_t patches, int H, int W) {
  const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t p = gid >> 4;
  if (p >= patches) return;
  const int t = (int)(gid & 15);
  const int gw = W >> 2, gh = H >> 2;
  const int px = (int)(p % gw), py = (int)((p / gw) % gh);
  const size_t b = p / ((size_t)gw * gh);
  f32x4_t v = f32x4_t{0.f, 0.f, 0.f, 0.f};
  if (t < 12) v = *(const f32x4_t*)(img + ((b * 3 + (t >> 2)) * H + (py * 4 + (t & 3))) * (size_t)W + px * 4);
  store4h<E>(out + p * 64 + t * 4, v);
}

template <class E>
void launch_dwconv(const float* x, const float* w, const float* bias, const float* g, const float* b, void* out, int B, int H, int W,
                   int C, float eps, hipStream_t s) {
  const int CG = C / 4;
  int PG = 1;
  while (PG * 2 * CG <= 256) PG *= 2;
  if (PG > 256 / RUN) PG = 256 / RUN;                    // PG * RUN <= 256: every pixel of the block has a reducing thread
  const int xblocks = (W + PG * RUN - 1) / (PG * RUN);
  hipLaunchKernelGGL((dwconv7_ln_kernel<E>), dim3((unsigned)(B * H * xblocks)), dim3(256), 0, s, x, w, bias, g, b, (E*)out, H, W, C,
                     PG, xblocks, eps);
}

template <class E>
void launch_patchify(const float* x, const float* g, const float* b, void* out, int M, int H, int W, int C, float eps, hipStream_t s) {
  dim3 grid((M + 3) / 4), block(256);
  const int mj = (C + 255) / 256;
  if (mj <= 1) hipLaunchKernelGGL((ln_patchify2_kernel<E, 1>), grid, block, 0, s, x, g, b, (E*)out, M, H, W, C, eps);
  else if (mj <= 2) hipLaunchKernelGGL((ln_patchify2_kernel<E, 2>), grid, block, 0, s, x, g, b, (E*)out, M, H, W, C, eps);
  else hipLaunchKernelGGL((ln_patchify2_kernel<E, 4>), grid, block, 0, s, x, g, b, (E*)out, M, H, W, C, eps);
}

bool misaligned(const void* p) { return ((uintptr_t)p & 15) != 0; }
constexpr long long MAX_ELEMS = 1ll << 31;               // element offsets of one tensor stay inside 32 bits of pixels x channels

}  // namespace

extern "C" int hm_dwconv7_ln(const float* x, const float* w, const float* bias, const float* gamma, const float* beta, void* out,
                             int B, int H, int W, int C, float eps, int dtype, void* stream) {
  if (!x || !w || !bias || !gamma || !beta || !out) return hm_set_error(HM_ERR_ARG, "hm_dwconv7_ln: null pointer");
  if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || C % 4 != 0 || C > 1024)
    return hm_set_error(HM_ERR_ARG, "hm_dwconv7_ln: need B, H, W > 0, 0 < C <= 1024, C % 4 == 0");
  if ((long long)B * H * W >= MAX_ELEMS / 4) return hm_set_error(HM_ERR_ARG, "hm_dwconv7_ln: B * H * W too large");
  if (misaligned(x) || misaligned(w) || misaligned(bias) || misaligned(gamma) || misaligned(beta) || ((uintptr_t)out & 7))
    return hm_set_error(HM_ERR_ARG, "hm_dwconv7_ln: pointers must be 16-byte aligned (out: 8)");
  if (dtype != HM_DTYPE_BF16 && dtype != HM_DTYPE_F16) return hm_set_error(HM_ERR_ARG, "hm_dwconv7_ln: dtype must be HM_DTYPE_BF16 or HM_DTYPE_F16");
  hipStream_t s = (hipStream_t)stream;
  HmProfScope prof(HM_K_OTHER, 120, B * H * W, C, 49, s);
  if (dtype == HM_DTYPE_BF16) launch_dwconv<__bf16>(x, w, bias, gamma, beta, out, B, H, W, C, eps, s);
  else launch_dwconv<_Float16>(x, w, bias, gamma, beta, out, B, H, W, C, eps, s);
  return hm_check_launch("hm_dwconv7_ln");
}

extern "C" int hm_ln_patchify2(const float* x, const float* gamma, const float* beta, void* out, int B, int H, int W, int C, float eps,
                               int dtype, void* stream) {
  if (!x || !gamma || !beta || !out) return hm_set_error(HM_ERR_ARG, "hm_ln_patchify2: null pointer");
  if (B <= 0 || H <= 0 || W <= 0 || (H & 1) || (W & 1) || C <= 0 || C % 4 != 0 || C > 1024)
    return hm_set_error(HM_ERR_ARG, "hm_ln_patchify2: need B > 0, even H and W, 0 < C <= 1024, C % 4 == 0");
  if ((long long)B * H * W >= MAX_ELEMS / 4) return hm_set_error(HM_ERR_ARG, "hm_ln_patchify2: B * H * W too large");
  if (misaligned(x) || misaligned(gamma) || misaligned(beta) || ((uintptr_t)out & 7))
    return hm_set_error(HM_ERR_ARG, "hm_ln_patchify2: pointers must be 16-byte aligned (out: 8)");
  if (dtype != HM_DTYPE_BF16 && dtype != HM_DTYPE_F16) return hm_set_error(HM_ERR_ARG, "hm_ln_patchify2: dtype must be HM_DTYPE_BF16 or HM_DTYPE_F16");
  hipStream_t s = (hipStream_t)stream;
  HmProfScope prof(HM_K_LAYERNORM, 121, B * H * W, C, 0, s);
  if (dtype == HM_DTYPE_BF16) launch_patchify<__bf16>(x, gamma, beta, out, B * H * W, H, W, C, eps, s);
  else launch_patchify<_Float16>(x, gamma, beta, out, B * H * W, H, W, C, eps, s);
  return hm_check_launch("hm_ln_patchify2");
}

extern "C" int hm_stem4_im2col(const float* img, void* patches, int B, int H, int W, int dtype, void* stream) {
  if (!img || !patches) return hm_set_error(HM_ERR_ARG, "hm_stem4_im2col: null pointer");
  if (B <= 0 || H <= 0 || W <= 0 || H % 4 != 0 || W % 4 != 0) return hm_set_error(HM_ERR_ARG, "hm_stem4_im2col: need B > 0, H % 4 == 0, W % 4 == 0");
  if ((long long)B * H * W >= MAX_ELEMS / 4) return hm_set_error(HM_ERR_ARG, "hm_stem4_im2col: B * H * W too large");
  if (misaligned(img) || ((uintptr_t)patches & 7)) return hm_set_error(HM_ERR_ARG, "hm_stem4_im2col: img must be 16-byte aligned (patches: 8)");
  if (dtype != HM_DTYPE_BF16 && dtype != HM_DTYPE_F16) return hm_set_error(HM_ERR_ARG, "hm_stem4_im2col: dtype must be HM_DTYPE_BF16 or HM_DTYPE_F16");
  hipStream_t s = (hipStream_t)stream;
  const size_t np = (size_t)B * (H / 4) * (W / 4);
  HmProfScope prof(HM_K_IM2COL, 122, (int)np, 64, 0, s);
  const unsigned grid = (unsigned)((np * 16 + 255) / 256);
  if (dtype == HM_DTYPE_BF16) hipLaunchKernelGGL((stem4_im2col_kernel<__bf16>), dim3(grid), dim3(256), 0, s, img, (__bf16*)patches, np, H, W);
  else hipLaunchKernelGGL((stem4_im2col_kernel<_Float16>), dim3(grid), dim3(256), 0, s, img, (_Float16*)patches, np, H, W);
  return hm_check_launch("hm_stem4_im2col");
}
