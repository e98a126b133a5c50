// hm_crop_batch_aa - the crop of prepare_item (infer.py:263-352): hm_crop_batch with the anti-alias prefilter of upstream
// HaMeR's demo dataset.  A hand whose crop is shrunk by more than 2.2x (df = (S / P) / 2 > 1.1) samples the frame blurred by
// skimage.filters.gaussian(sigma = (df - 1) / 2, preserve_range=True) -- scipy.ndimage.gaussian_filter, mode 'nearest',
// truncate 4 -- with cv2.warpAffine's bilinear taps in floating point; every other hand takes hm_crop_batch's 8-bit rule.
//
// Blur and bilinear blend are both separable, so one output pixel is  sum_i WY[i] sum_j WX[j] frame[i][j]  with the axis
// weights  W[t] = a0 g[|t|] + a1 g[|t - 1|],  t = -r .. r + 1  around the pixel's integer source coordinate (a0, a1: the
// two bilinear weights of the axis, 0 where that tap lies outside the frame; g: the normalised Gaussian taps); the frame's
// replicated edge is a clamp of the index i or j.  One workgroup owns one output row of one hand: WY is the same for the
// whole row, so the VERTICAL pass runs once per source column of the row's footprint -- lanes walk consecutive bytes of
// 2r + 2 frame rows -- and leaves fp32 column sums in LDS, 256 columns at a time; every lane then adds the columns of the
// chunk that fall into its own window with its WX.  No blurred frame and no per-hand frame copy exists in HBM; the work is
// (footprint width) x (2r + 2) frame bytes per output row, not (2r + 2)^2 per output pixel.
#include <math.h>
#include <stdio.h>
#include "common.h"
#include "hamer_hip_internal.h"

namespace {

constexpr int AB_BITS = 10, INTER_BITS = 5, INTER_TAB = 32;
constexpr int RMAX = HM_CROP_AA_MAX_RADIUS, NTAPS = HM_CROP_AA_TAPS;
constexpr int CHUNK = 256;                       // source columns per pass through LDS (x 3 channels = 3 bytes per lane)

// hm_crop_batch's pixel (patch.hip crop_kernel), the same integer arithmetic: same bytes
__device__ __forceinline__ void crop_pixel_u8(const uint8_t* __restrict__ frame, int H, int W, double m0, double m4, int x0,
                                              int y0, int xs, int y, float* bgr) {
  const int adelta = (int)rint(m0 * (double)xs * 1024.0);
  const int bdelta = (int)rint(m4 * (double)y * 1024.0);
  const int X = (x0 + adelta) >> (AB_BITS - INTER_BITS);
  const int Y = (y0 + bdelta) >> (AB_BITS - INTER_BITS);
  const int sx = X >> INTER_BITS, sy = Y >> INTER_BITS;
  const int fx = X & (INTER_TAB - 1), fy = Y & (INTER_TAB - 1);
  const int w00 = (INTER_TAB - fx) * (INTER_TAB - fy), w01 = fx * (INTER_TAB - fy);
  const int w10 = (INTER_TAB - fx) * fy, w11 = fx * fy;
  const bool x0ok = sx >= 0 && sx < W, x1ok = sx + 1 >= 0 && sx + 1 < W;
  const bool y0ok = sy >= 0 && sy < H, y1ok = sy + 1 >= 0 && sy + 1 < H;
  int acc[3] = {512, 512, 512};
  if (y0ok && x0ok) { const uint8_t* p = frame + ((size_t)sy * W + sx) * 3; acc[0] += w00 * p[0]; acc[1] += w00 * p[1]; acc[2] += w00 * p[2]; }
  if (y0ok && x1ok) { const uint8_t* p = frame + ((size_t)sy * W + sx + 1) * 3; acc[0] += w01 * p[0]; acc[1] += w01 * p[1]; acc[2] += w01 * p[2]; }
  if (y1ok && x0ok) { const uint8_t* p = frame + ((size_t)(sy + 1) * W + sx) * 3; acc[0] += w10 * p[0]; acc[1] += w10 * p[1]; acc[2] += w10 * p[2]; }
  if (y1ok && x1ok) { const uint8_t* p = frame + ((size_t)(sy + 1) * W + sx + 1) * 3; acc[0] += w11 * p[0]; acc[1] += w11 * p[1]; acc[2] += w11 * p[2]; }
  bgr[0] = (float)(acc[0] >> 10); bgr[1] = (float)(acc[1] >> 10); bgr[2] = (float)(acc[2] >> 10);
}

// g[|k|], 0 beyond the radius (g: the hand's taps in LDS)
__device__ __forceinline__ float tap_at(const float* g, int k, int r) {
  k = k < 0 ? -k : k;
  return k <= r ? g[k] : 0.0f;
}

__global__ __launch_bounds__(256) void crop_aa_kernel(const uint8_t* __restrict__ frame, int H, int W,
                                                      const hm_crop_aa_box* __restrict__ boxes, const float* __restrict__ taps,
                                                      float* __restrict__ out, int P, float m0, float m1, float m2, float s0,
                                                      float s1, float s2) {
  __shared__ float g[NTAPS];
  __shared__ float wy[2 * RMAX + 2];
  __shared__ int row[2 * RMAX + 2];
  __shared__ float col[2][CHUNK * 3];

  const int b = blockIdx.z, y = blockIdx.y, tid = threadIdx.x;
  const int l = blockIdx.x * 256 + tid;              // column of the patch BEFORE the mirror: source x grows with the lane
  const bool live = l < P;
  const hm_crop_aa_box bx = boxes[b];
  const int xo = bx.flip ? (P - 1 - l) : l;          // cv2.flip(patch, 1) after the crop (infer.py:331)
  float* o = out + (size_t)b * 3 * P * P + (size_t)y * P + xo;
  const size_t plane = (size_t)P * P;
  const int r = bx.radius;

  float bgr[3] = {0.0f, 0.0f, 0.0f};
  if (r < 0 || r > RMAX) {                           // not a record of hm_crop_aa_box_from_bbox: say so in the pixels
    if (live) { o[0] = NAN; o[plane] = NAN; o[2 * plane] = NAN; }
    return;
  }
  if (bx.sigma == 0.0f) {                            // df <= 1.1: the 8-bit rule
    if (!live) return;
    crop_pixel_u8(frame, H, W, bx.m0, bx.m4, bx.x0, bx.y0, l, y, bgr);
  } else {
    // ---- this row's vertical weights and frame rows (the same for every lane)
    const int Y = (bx.y0 + (int)rint(bx.m4 * (double)y * 1024.0)) >> (AB_BITS - INTER_BITS);
    const int sy = Y >> INTER_BITS, fy = Y & (INTER_TAB - 1);
    const float b0 = (sy >= 0 && sy < H) ? (float)(INTER_TAB - fy) * (1.0f / INTER_TAB) : 0.0f;
    const float b1 = (sy + 1 >= 0 && sy + 1 < H) ? (float)fy * (1.0f / INTER_TAB) : 0.0f;
    const int nt = 2 * r + 2;
    if (tid < NTAPS) g[tid] = taps[(size_t)b * NTAPS + tid];
    __syncthreads();
    if (tid < nt) {
      const int t = tid - r;
      wy[tid] = b0 * tap_at(g, t, r) + b1 * tap_at(g, t - 1, r);
      row[tid] = min(max(sy + t, 0), H - 1);
    }
    // ---- this lane's horizontal taps
    const int X = (bx.x0 + (int)rint(bx.m0 * (double)l * 1024.0)) >> (AB_BITS - INTER_BITS);
    const int sx = X >> INTER_BITS, fx = X & (INTER_TAB - 1);
    const float a0 = (live && sx >= 0 && sx < W) ? (float)(INTER_TAB - fx) * (1.0f / INTER_TAB) : 0.0f;
    const float a1 = (live && sx + 1 >= 0 && sx + 1 < W) ? (float)fx * (1.0f / INTER_TAB) : 0.0f;
    const bool any = a0 != 0.0f || a1 != 0.0f;
    // ---- the source columns the workgroup needs: first lane's window .. last live lane's, and no further out of the frame
    // than a window with a tap inside it reaches
    const int l0 = blockIdx.x * 256, l1 = min(l0 + 255, P - 1);
    const int sx_lo = ((bx.x0 + (int)rint(bx.m0 * (double)l0 * 1024.0)) >> (AB_BITS - INTER_BITS)) >> INTER_BITS;
    const int sx_hi = ((bx.x0 + (int)rint(bx.m0 * (double)l1 * 1024.0)) >> (AB_BITS - INTER_BITS)) >> INTER_BITS;
    const int j_lo = max(min(sx_lo, sx_hi) - r, -1 - r), j_hi = min(max(sx_lo, sx_hi) + r + 1, W + r);
    __syncthreads();
    if (b0 != 0.0f || b1 != 0.0f) {                  // (else the whole row samples outside the frame: 0)
      const size_t pitch = (size_t)W * 3;
      int buf = 0;
      for (int cb = j_lo; cb <= j_hi; cb += CHUNK, buf ^= 1) {
        // vertical pass: column sums of CHUNK source columns x 3 channels, lanes on consecutive bytes of a frame row; a lane's
        // three bytes (256 apart) go through the rows together, so their loads are in flight at the same time
        size_t at[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const int e = tid + 256 * k;
          at[k] = (size_t)min(max(cb + e / 3, 0), W - 1) * 3 + (e % 3);
        }
        float v[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll 4
        for (int u = 0; u < nt; ++u) {
          const uint8_t* p = frame + (size_t)row[u] * pitch;
          const float w = wy[u];
          v[0] = fmaf(w, (float)p[at[0]], v[0]); v[1] = fmaf(w, (float)p[at[1]], v[1]); v[2] = fmaf(w, (float)p[at[2]], v[2]);
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) col[buf][tid + 256 * k] = v[k];       // (columns past j_hi: a clamped read nobody uses)
        __syncthreads();      // (one barrier per chunk: the next pass writes the OTHER buffer, which every lane left before this barrier)
        // horizontal pass: the part of this lane's window that lies in the chunk, in ascending source order
        if (any) {
          const int ja = max(sx - r, cb), jb = min(sx + r + 1, min(cb + CHUNK - 1, j_hi));
          for (int j = ja; j <= jb; ++j) {
            const int t = j - sx;
            const float w = a0 * tap_at(g, t, r) + a1 * tap_at(g, t - 1, r);
            const float* c = &col[buf][(j - cb) * 3];
            bgr[0] = fmaf(w, c[0], bgr[0]); bgr[1] = fmaf(w, c[1], bgr[1]); bgr[2] = fmaf(w, c[2], bgr[2]);
          }
        }
      }
    }
    if (!live) return;
  }
  o[0] = (bgr[2] - m0) / s0;                         // channel 0 = R (BGR -> RGB, infer.py:329)
  o[plane] = (bgr[1] - m1) / s1;
  o[2 * plane] = (bgr[0] - m2) / s2;
}

}  // namespace

// Host helper: hm_crop_box_from_bbox's matrix arithmetic plus the size rule of prepare_item (infer.py:314-316) and the taps
// of scipy.ndimage's _gaussian_kernel1d (what skimage.filters.gaussian runs), all in double.
extern "C" int hm_crop_aa_box_from_bbox(double cx, double cy, double size, int flip, int P, hm_crop_aa_box* out,
                                        float* taps_out) {
  if (!out || !taps_out) return hm_set_error(HM_ERR_ARG, "hm_crop_aa_box_from_bbox: null pointer");
  hm_crop_box bx;
  const int rc = hm_crop_box_from_bbox(cx, cy, size, flip, P, &bx);
  if (rc != HM_OK) return rc;
  out->m0 = bx.m0; out->m4 = bx.m4; out->x0 = bx.x0; out->y0 = bx.y0; out->flip = bx.flip; out->reserved = 0;
  out->sigma = 0.0f; out->radius = 0; out->pad[0] = out->pad[1] = 0;
  for (int k = 0; k < NTAPS; ++k) taps_out[k] = 0.0f;
  taps_out[0] = 1.0f;
  const double df = (size / (double)P) / 2.0;
  if (!(df > 1.1)) return HM_OK;
  const double sigma = (df - 1.0) / 2.0;
  if (!(sigma <= HM_CROP_AA_MAX_SIGMA)) {             // (radius 48 ends at sigma 12.125; the supported range ends at 12)
    char msg[160];
    snprintf(msg, sizeof msg, "hm_crop_aa_box_from_bbox: crop size %.6g at P = %d needs a blur of sigma %.6g, above %g (radius %d)",
             size, P, sigma, HM_CROP_AA_MAX_SIGMA, RMAX);
    return hm_set_error(HM_ERR_ARG, msg);
  }
  const int r = (int)(4.0 * sigma + 0.5);
  double gd[NTAPS], sum = 0.0;
  const double c = -0.5 / (sigma * sigma);
  for (int k = 0; k <= r; ++k) gd[k] = exp(c * (double)(k * k));
  for (int k = -r; k <= r; ++k) sum += gd[k < 0 ? -k : k];
  for (int k = 0; k <= r; ++k) taps_out[k] = (float)(gd[k] / sum);
  out->sigma = (float)sigma; out->radius = r;
  return HM_OK;
}

extern "C" int hm_crop_batch_aa(const uint8_t* frame, int H, int W, const hm_crop_aa_box* boxes, const float* taps, float* out,
                                int B, int P, const float* mean3_host, const float* std3_host, void* stream_) {
  if (!frame || !boxes || !taps || !out || !mean3_host || !std3_host) return hm_set_error(HM_ERR_ARG, "hm_crop_batch_aa: null pointer");
  if (H <= 0 || W <= 0 || B <= 0 || P <= 0 || B > 65535 || P > 65535) return hm_set_error(HM_ERR_ARG, "hm_crop_batch_aa: bad sizes");
  dim3 grid((P + 255) / 256, P, B), block(256);
  HmProfScope prof(HM_K_CROP, 1, B, P, P, (hipStream_t)stream_);
  hipLaunchKernelGGL(crop_aa_kernel, grid, block, 0, (hipStream_t)stream_, frame, H, W, boxes, taps, out, P, mean3_host[0],
                     mean3_host[1], mean3_host[2], std3_host[0], std3_host[1], std3_host[2]);
  return hm_check_launch("hm_crop_batch_aa");
}
