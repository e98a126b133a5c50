// hm_conv2d_nhwc for HM_DTYPE_F32: the YOLOv7 convolutions in fp32 operands (the reference's CPU branch, detector.py:110-112
// with half = False), as an implicit GEMM on the fp32-input MFMA.
//   rows (M)    : output pixels n*Hout*Wout (NHWC, pixel stride ldy), 32 per MFMA block
//   columns (N) : output channels, 32 per MFMA block
//   K           : (ky, kx, ci) as the 16-bit route lays out its weights, zero padded to Kpad (% 64 == 0)
// v_mfma_f32_32x32x2_f32 (cdna_hip_programming.md §3 'FP32-input MFMA'): f32 in, f32 accumulate, bit-for-bit a k-ordered fmaf
// chain; 64 cycles issue and dependent latency per SIMD (MI355X_MICROARCH.md, MFMA cycle table), so the 2 x 2 independent 32x32
// accumulators of a wave keep the pipe busy from one wave per SIMD.  157 TF/s peak = the f32 vector rate, 1/16 of the 16-bit MFMA.
//
// Numerics contract: every output is bias + (a sum over K in ONE fixed order that depends on k*k*Cin only): no split-K, no K groups,
// no tile-dependent reduction.  An output's value therefore does not depend on the tile shape, the grid, the batch it rides in or
// its place in that batch -- the fp32 route is deterministic and batch-invariant by construction.
//
// Tiles: 256 threads = 4 waves; a wave owns RB x CB blocks of 32x32.  K moves in stages of 32 fp32: every thread fetches its
// float4 pieces of the next stage into registers (dwordx4 loads, in flight while the MFMAs run), then writes them to the other
// half of a double-buffered LDS tile -- one barrier per stage.  LDS rows are 32 + 4 floats (144 B): 16-byte aligned for
// ds_read_b128, and the 32 rows one MFMA operand read touches start in different banks.
// Within a stage the K order is: for each group g of 8 k, lanes 0-31 (k-slot 0 of the MFMA) hold k = 8g + e and lanes 32-63
// (k-slot 1) hold k = 8g + 4 + e, e = 0..3 the MFMA's index in the group -- one 16-byte LDS read per operand and group, the
// same mapping on both operands.  (That MFMA side of a stage lives in mfma_f32_tile.h, shared with gemm_f32.hip.)
#include <math.h>
#include <stdio.h>
#include "common.h"
#include "hamer_hip_internal.h"
#include "mfma_f32_tile.h"      // F32_BK, F32_LDK and the MFMA side of the stage loop, shared with gemm_f32.hip

namespace {

struct ConvF32Args {
  const float* X;      // [N][H][Wd][ldx], already offset to the first input channel
  const float* W;      // [Cout][Kpad]
  const float* bias;   // [Cout]
  float* Y;            // [M][ldy], already offset to the channel slice
  int H, Wd, Hout, Wout, Cin, cin_log2, ksz, stride, pad, taps, ldx, ldy, Kpad, nk, M, Cout, act;
  const float* R;      // EPI_RELU only: optional [M][ldr] residual, added before the ReLU
  int ldr;
};

// epilogues: EPI_YOLO is hm_conv2d_nhwc's (act 1: SiLU, act 0: none); EPI_RELU is hm_conv2d_f32_relu's (the ResNet-34 of the
// RootNet backbone: + optional residual, then ReLU when act == 2).  Both apply to the same k-ordered sum.
enum { EPI_YOLO = 0, EPI_RELU = 1 };

template <int WM, int WN, int RB, int CB>
constexpr int conv_f32_lds_bytes() { return 2 * (WM * RB * 32 + WN * CB * 32) * F32_LDK * 4; }

template <int WM, int WN, int RB, int CB, int EPI>
__global__ __launch_bounds__(256) void conv_f32_kernel(ConvF32Args a) {
  static_assert(WM * WN == 4, "4 waves");
  constexpr int BM = WM * RB * 32, BN = WN * CB * 32;
  constexpr int AL = BM / 32, BL = BN / 32;         // float4 pieces per thread and stage: 8 per tile row, 32 rows per pass
  constexpr int STAGE = (BM + BN) * F32_LDK;         // floats per LDS buffer
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave % WM, wn = wave / WM;
  const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;
  const int q = tid & 7, r0 = tid >> 3;

  // the A rows this thread fetches: image base and the input coordinate of tap (0, 0); a row past M gets a coordinate that
  // every bounds test rejects, so it reads zeros and is never stored
  const float* abase[AL];
  int aiy[AL], aix[AL];
#pragma unroll
  for (int i = 0; i < AL; ++i) {
    const int m = m0 + r0 + 32 * i;
    abase[i] = a.X;
    aiy[i] = -(1 << 28); aix[i] = 0;
    if (m < a.M) {
      const int ox = m % a.Wout, t = m / a.Wout, oy = t % a.Hout, n = t / a.Hout;
      abase[i] = a.X + (size_t)n * a.H * a.Wd * a.ldx;
      aiy[i] = oy * a.stride - a.pad; aix[i] = ox * a.stride - a.pad;
    }
  }
  const float* brow[BL];
  bool bok[BL];
#pragma unroll
  for (int i = 0; i < BL; ++i) {
    const int co = n0 + r0 + 32 * i;
    bok[i] = co < a.Cout;
    brow[i] = a.W + (size_t)(bok[i] ? co : 0) * a.Kpad + 4 * q;
  }

  f32x4_t ra[AL], rb[BL];
  auto fetch = [&](int kb) {
    const int k0 = kb + 4 * q;                       // 4 consecutive k of one tap (Cin >= 8, a power of two)
    const int tap = k0 >> a.cin_log2, ci = k0 & (a.Cin - 1);
    const int ky = tap / a.ksz, kx = tap - ky * a.ksz;
    const bool tap_ok = tap < a.taps;                // K padding: zeros
#pragma unroll
    for (int i = 0; i < AL; ++i) {
      const int iy = aiy[i] + ky, ix = aix[i] + kx;
      ra[i] = f32x4_t{0.f, 0.f, 0.f, 0.f};
      if (tap_ok && (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.Wd)
        ra[i] = *(const f32x4_t*)(abase[i] + ((size_t)iy * a.Wd + ix) * a.ldx + ci);
    }
#pragma unroll
    for (int i = 0; i < BL; ++i) {
      rb[i] = f32x4_t{0.f, 0.f, 0.f, 0.f};
      if (bok[i]) rb[i] = *(const f32x4_t*)(brow[i] + kb);
    }
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
  const int brow_l = f32_tile_lane_offset(BM + wn * CB * 32, lane);
  const int nk = a.nk;
  fetch(0);
  stash(0);
  __syncthreads();
  for (int st = 0; st < nk; ++st) {
    const int cur = st & 1;
    if (st + 1 < nk) fetch((st + 1) * F32_BK);
    f32_tile_stage<RB, CB>(smem + cur * STAGE, arow, brow_l, acc);
    if (st + 1 < nk) stash(cur ^ 1);
    __syncthreads();
  }

  // epilogue: 32x32 C/D map -- column (output channel) = lane & 31, row (pixel) = (r & 3) + 8 (r >> 2) + 4 (lane >> 5);
  // 32 lanes store 128 contiguous bytes of one pixel
#pragma unroll
  for (int j = 0; j < CB; ++j) {
    const int co = n0 + (wn * CB + j) * 32 + (lane & 31);
    if (co >= a.Cout) continue;
    const float b = a.bias[co];
#pragma unroll
    for (int i = 0; i < RB; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = m0 + (wm * RB + i) * 32 + f32_tile_row(r, lane);
        if (m >= a.M) continue;
        float v = acc[i][j][r] + b;
        if constexpr (EPI == EPI_YOLO) {
          if (a.act) v = v / (1.0f + expf(-v));      // SiLU as torch's CPU kernel writes it: x / (1 + exp(-x)), IEEE division
        } else {
          if (a.R) v += a.R[(size_t)m * a.ldr + co];  // BasicBlock: bn2(conv2(x)) + identity, then ReLU
          if (a.act) v = v > 0.f ? v : 0.f;
        }
        a.Y[(size_t)m * a.ldy + co] = v;
      }
  }
}

template <int WM, int WN, int RB, int CB, int EPI>
int launch_conv_f32(const ConvF32Args& g, hipStream_t s) {
  constexpr int BM = WM * RB * 32, BN = WN * CB * 32, LDS = conv_f32_lds_bytes<WM, WN, RB, CB>();
  auto kern = conv_f32_kernel<WM, WN, RB, CB, EPI>;
  static HmLdsOnce lds_once;
  if (const int rc = lds_once.ensure((const void*)kern, LDS, "hm_conv2d_nhwc (fp32): cannot raise the dynamic LDS limit")) return rc;
  hipLaunchKernelGGL(kern, dim3((unsigned)((g.M + BM - 1) / BM), (unsigned)((g.Cout + BN - 1) / BN)), dim3(256), LDS, s, g);
  return hm_check_launch(EPI == EPI_YOLO ? "hm_conv2d_nhwc (fp32)" : "hm_conv2d_f32_relu");
}

// the tile changes which threads compute an output, never its arithmetic (see the numerics contract above)
template <int EPI>
int dispatch_conv_f32(const ConvF32Args& g, hipStream_t stream) {
  if (g.Cout <= 32) return launch_conv_f32<4, 1, 2, 1, EPI>(g, stream);                  // 256 x 32: Conv 0 (32), the detect heads (24)
  if (g.Cout <= 64) return launch_conv_f32<4, 1, 2, 2, EPI>(g, stream);                  // 256 x 64
  const long tiles = (long)((g.M + 127) / 128) * ((g.Cout + 127) / 128);
  if (tiles < hm_device_cu_count()) return launch_conv_f32<2, 2, 1, 1, EPI>(g, stream);  // 64 x 64: the small maps of one frame
  return launch_conv_f32<2, 2, 2, 2, EPI>(g, stream);                                    // 128 x 128
}

// the checks both entry points share, in two parts (the entry point's own act / resid checks go between them, as
// hm_conv2d_nhwc always ordered them); `what` names the entry point in the error string
int conv_f32_fail(const char* what, const char* why) {
  char msg[192];
  snprintf(msg, sizeof msg, "%s: %s", what, why);
  return hm_set_error(HM_ERR_ARG, msg);
}

int conv_f32_check_shape(const hm_conv_args& c, const char* what) {
  if (!c.X || !c.W || !c.Y || !c.bias) return conv_f32_fail(what, "null operand");
  if (c.N <= 0 || c.H <= 0 || c.W_in <= 0 || c.Cin <= 0 || c.Cout <= 0) return conv_f32_fail(what, "empty problem");
  if ((c.ksize != 1 && c.ksize != 3 && c.ksize != 5 && c.ksize != 7) || (c.stride != 1 && c.stride != 2))
    return conv_f32_fail(what, "kernel size 1, 3, 5 or 7, stride 1 or 2");
  return HM_OK;
}

int conv_f32_args(const hm_conv_args& c, const char* what, ConvF32Args& g) {
  int lg = 0;
  while ((1 << lg) < c.Cin) ++lg;
  if ((1 << lg) != c.Cin || c.Cin < 8) return conv_f32_fail(what, "Cin must be a power of two >= 8");
  const int taps = c.ksize * c.ksize;
  if (c.Kpad % 64 != 0 || c.Kpad < taps * c.Cin) return conv_f32_fail(what, "Kpad must be a multiple of 64 covering k*k*Cin");
  if (c.ldx % 4 != 0 || c.ldx < c.Cin || c.ldy < c.Cout) return conv_f32_fail(what, "ldx % 4 == 0, ldx >= Cin, ldy >= Cout");
  if ((((uintptr_t)c.X | (uintptr_t)c.W) & 15) || (((uintptr_t)c.Y | (uintptr_t)c.bias) & 3))
    return conv_f32_fail(what, "X / W 16-byte aligned, Y / bias 4-byte aligned");
  const int pad = c.ksize / 2;
  const int Hout = (c.H + 2 * pad - c.ksize) / c.stride + 1, Wout = (c.W_in + 2 * pad - c.ksize) / c.stride + 1;
  if ((size_t)c.N * Hout * Wout >= (1ull << 31) || (size_t)c.N * c.H * c.W_in >= (1ull << 31)) return conv_f32_fail(what, "more than 2^31 pixels");
  g = ConvF32Args{};
  g.X = (const float*)c.X; g.W = (const float*)c.W; g.bias = c.bias; g.Y = (float*)c.Y;
  g.H = c.H; g.Wd = c.W_in; g.Hout = Hout; g.Wout = Wout; g.Cin = c.Cin; g.cin_log2 = lg; g.ksz = c.ksize; g.stride = c.stride;
  g.pad = pad; g.taps = taps; g.ldx = c.ldx; g.ldy = c.ldy; g.Kpad = c.Kpad; g.M = c.N * Hout * Wout; g.Cout = c.Cout;
  g.nk = (taps * c.Cin + F32_BK - 1) / F32_BK;       // stages up to k*k*Cin: the zero tail of Kpad adds nothing (Conv 0: 72 -> 96, not 128)
  g.act = c.act;
  return HM_OK;
}

}  // namespace

int hm_conv2d_f32(const hm_conv_args* a, hipStream_t stream) {
  const hm_conv_args& c = *a;
  if (const int rc = conv_f32_check_shape(c, "hm_conv2d_nhwc (fp32)")) return rc;
  if (c.act < 0 || c.act > 1 || c.resid || (c.out_f32 && c.act))
    return hm_set_error(HM_ERR_ARG, "hm_conv2d_nhwc (fp32): act is 0 or 1 (SiLU), no resid / ReLU");
  ConvF32Args g;
  if (const int rc = conv_f32_args(c, "hm_conv2d_nhwc (fp32)", g)) return rc;
  HmProfScope prof(HM_K_CONV, c.ksize * 10 + c.stride, g.M, g.Cout, g.taps * c.Cin, stream);
  return dispatch_conv_f32<EPI_YOLO>(g, stream);
}

extern "C" int hm_conv2d_f32_relu(const hm_conv_args* a, void* stream_) {
  if (!a) return hm_set_error(HM_ERR_ARG, "hm_conv2d_f32_relu: null args");
  const hm_conv_args& c = *a;
  if (c.dtype != HM_DTYPE_F32) return hm_set_error(HM_ERR_ARG, "hm_conv2d_f32_relu: dtype must be HM_DTYPE_F32");
  if (const int rc = conv_f32_check_shape(c, "hm_conv2d_f32_relu")) return rc;
  if ((c.act != 0 && c.act != 2) || c.out_f32) return hm_set_error(HM_ERR_ARG, "hm_conv2d_f32_relu: act is 0 or 2 (ReLU), out_f32 is 0");
  if (c.resid && (c.ldr < c.Cout || ((uintptr_t)c.resid & 3)))
    return hm_set_error(HM_ERR_ARG, "hm_conv2d_f32_relu: resid needs ldr >= Cout and 4-byte alignment");
  ConvF32Args g;
  if (const int rc = conv_f32_args(c, "hm_conv2d_f32_relu", g)) return rc;
  g.R = (const float*)c.resid;
  g.ldr = c.ldr;
  g.act = c.act == 2;
  hipStream_t stream = (hipStream_t)stream_;
  HmProfScope prof(HM_K_CONV, c.ksize * 10 + c.stride, g.M, g.Cout, g.taps * c.Cin, stream);
  return dispatch_conv_f32<EPI_RELU>(g, stream);
}
