// Test-time augmentation of the YOLOv7 detector (Model.forward(x, augment=True), yolo.py:589-605): the network runs on the
// letterboxed input at scales 1, 0.83 and 0.67, the middle one mirrored left-right, and the three predictions, de-scaled
// and de-flipped, go to one NMS.  Two pieces are needed around the planned graphs:
//   hm_tta_scale             scale_img (utils/torch_utils.py:247-257) on the engine's [nb][h][w][8] image: the flip, the
//                            bilinear resize (F.interpolate, align_corners=False) and the 0.447 padding to a multiple of gs
//   hm_yolo_decode_batch_tta hm_yolo_decode_batch, then xywh / scale and x = full_w - x (yolo.py:599-603)
// Both are byte work: a thread per output pixel / prediction row, one wide store each.
#include <math.h>
#include <string.h>
#include <type_traits>
#include "common.h"
#include "hamer_hip_internal.h"

namespace {

constexpr int TTA_MAX_SIDE = 16384;

// scale_img's sizes, in doubles as Python computes them: s = int(n * ratio), padded = ceil(n * ratio / gs) * gs
bool tta_sizes(int h, int w, double ratio, int gs, int* sh, int* sw, int* hp, int* wp) {
  if (h <= 0 || w <= 0 || gs <= 0 || h > TTA_MAX_SIDE || w > TTA_MAX_SIDE || gs > TTA_MAX_SIDE || !(ratio > 0.0) || !(ratio <= 1.0))
    return false;
  *sh = (int)((double)h * ratio); *sw = (int)((double)w * ratio);
  *hp = (int)ceil((double)h * ratio / gs) * gs; *wp = (int)ceil((double)w * ratio / gs) * gs;
  return *sh > 0 && *sw > 0;
}

// One axis of the table: tap 0, tap 1, weight 0, weight 1 (fp32 bits) for each of the `pn` padded outputs; outputs past
// the resized size `dn` are padding (taps -1, weights 0).  The arithmetic is torch's for a float tensor
// (area_pixel_compute_source_index, compute_source_index_and_lambda) as torch's kernels evaluate it: scale = in / out and
// d + 0.5 in fp32, then scale * (d + 0.5) - 0.5 as ONE fused multiply-add (torch's CPU kernels are built with FMA
// contraction, its GPU kernels too), which moves a weight by up to 6e-5 at index ~640 against two roundings.
void tta_axis(int sn, int dn, int pn, int flip, int32_t* t) {
  const float scale = (float)sn / (float)dn;
  for (int d = 0; d < pn; ++d) {
    int i0 = -1, i1 = -1;
    float l0 = 0.0f, l1 = 0.0f;
    if (d < dn) {
      float src = fmaf(scale, (float)d + 0.5f, -0.5f);            // (one rounding, see above)
      if (src < 0.0f) src = 0.0f;
      i0 = (int)src;
      i1 = i0 + (i0 < sn - 1 ? 1 : 0);
      l1 = fminf(fmaxf(src - (float)i0, 0.0f), 1.0f);
      l0 = 1.0f - l1;
      if (flip) { i0 = sn - 1 - i0; i1 = sn - 1 - i1; }
    }
    t[d] = i0; t[pn + d] = i1;
    memcpy(&t[2 * pn + d], &l0, 4); memcpy(&t[3 * pn + d], &l1, 4);
  }
}

template <class E>
__global__ __launch_bounds__(256) void tta_scale_kernel(const E* __restrict__ x, E* __restrict__ y, const int32_t* __restrict__ tab,
                                                        int h, int w, int hp, int wp) {
  typedef __attribute__((ext_vector_type(8))) E vec8;
  typedef __attribute__((ext_vector_type(4))) E vec4;
  const int pix = blockIdx.x * 256 + threadIdx.x;
  if (pix >= hp * wp) return;
  x += (size_t)blockIdx.y * h * w * 8;                     // image blockIdx.y of the pass
  y += (size_t)blockIdx.y * hp * wp * 8;
  const int oy = pix / wp, ox = pix - oy * wp;
  const int32_t *tx = tab, *ty = tab + 4 * wp;
  const int x0 = tx[ox], y0 = ty[oy];
  float v[3] = {0.447f, 0.447f, 0.447f};                  // F.pad(.., value=0.447), torch_utils.py:257
  if (x0 >= 0 && y0 >= 0) {
    // (the table is built for this h, w; the clamps keep a foreign table inside the image)
    const int xa = min(x0, w - 1), xb = min(max(tx[wp + ox], 0), w - 1);
    const int ya = min(y0, h - 1), yb = min(max(ty[hp + oy], 0), h - 1);
    const float lx0 = __int_as_float(tx[2 * wp + ox]), lx1 = __int_as_float(tx[3 * wp + ox]);
    const float ly0 = __int_as_float(ty[2 * hp + oy]), ly1 = __int_as_float(ty[3 * hp + oy]);
    const E* ra = x + (size_t)ya * w * 8;
    const E* rb = x + (size_t)yb * w * 8;
    const vec4 a0 = *(const vec4*)(ra + (size_t)xa * 8), a1 = *(const vec4*)(ra + (size_t)xb * 8);
    const vec4 b0 = *(const vec4*)(rb + (size_t)xa * 8), b1 = *(const vec4*)(rb + (size_t)xb * 8);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float top = lx0 * (float)a0[c] + lx1 * (float)a1[c];
      const float bot = lx0 * (float)b0[c] + lx1 * (float)b1[c];
      v[c] = ly0 * top + ly1 * bot;
    }
  }
  vec8 o;
#pragma unroll
  for (int c = 0; c < 3; ++c) o[c] = (E)v[c];
#pragma unroll
  for (int c = 3; c < 8; ++c) o[c] = (E)0.0f;
  *(vec8*)(y + (size_t)pix * 8) = o;
}

// decode_kernel of yolo.hip, expression for expression (the first rows of a TTA pred are the plain pass's bytes), then the
// de-scale as an IEEE division -- torch divides a CPU tensor by the scalar, it does not multiply by a reciprocal -- and the
// de-flip.
__global__ __launch_bounds__(256) void decode_tta_kernel(const float* __restrict__ raw, int ldraw, float* __restrict__ pred,
                                                         int row0, int ny, int nx, int no, float stride, float a0w, float a0h,
                                                         float a1w, float a1h, float a2w, float a2h, size_t raw_img, size_t pred_img,
                                                         float scale, int flip_lr, float full_w) {
  const int gid = blockIdx.x * 256 + threadIdx.x;
  if (gid >= 3 * ny * nx) return;
  raw += (size_t)blockIdx.y * raw_img;
  pred += (size_t)blockIdx.y * pred_img;
  const int a = gid / (ny * nx), p = gid - a * ny * nx;
  const int y = p / nx, x = p - y * nx;
  const float aw = a == 0 ? a0w : (a == 1 ? a1w : a2w), ah = a == 0 ? a0h : (a == 1 ? a1h : a2h);
  const float* r = raw + (size_t)p * ldraw + a * no;
  float* o = pred + ((size_t)row0 + gid) * no;
  for (int c = 0; c < no; ++c) {
    const float s = 1.0f / (1.0f + expf(-r[c]));
    float v = s;
    if (c == 0) v = (s * 2.0f - 0.5f + (float)x) * stride;
    else if (c == 1) v = (s * 2.0f - 0.5f + (float)y) * stride;
    else if (c == 2) { const float t = s * 2.0f; v = __fmul_rn(__fmul_rn(t, t), aw); }
    else if (c == 3) { const float t = s * 2.0f; v = __fmul_rn(__fmul_rn(t, t), ah); }
    if (c < 4) v = __fdiv_rn(v, scale);
    if (c == 0 && flip_lr) v = __fsub_rn(full_w, v);
    o[c] = v;
  }
}

}  // namespace

extern "C" int hm_tta_sizes(int h, int w, double ratio, int gs, int* sizes4) {
  int sh, sw, hp, wp;
  if (!sizes4) return hm_set_error(HM_ERR_ARG, "hm_tta_sizes: null pointer");
  if (!tta_sizes(h, w, ratio, gs, &sh, &sw, &hp, &wp))
    return hm_set_error(HM_ERR_ARG, "hm_tta_sizes: need 0 < h, w, gs <= 16384, 0 < ratio <= 1 and a resized image of at least one pixel");
  sizes4[0] = sh; sizes4[1] = sw; sizes4[2] = hp; sizes4[3] = wp;
  return HM_OK;
}

extern "C" int hm_tta_tables(int h, int w, double ratio, int gs, int flip_lr, int32_t* tab) {
  int sh, sw, hp, wp;
  if (!tab) return hm_set_error(HM_ERR_ARG, "hm_tta_tables: null pointer");
  if (!tta_sizes(h, w, ratio, gs, &sh, &sw, &hp, &wp))
    return hm_set_error(HM_ERR_ARG, "hm_tta_tables: need 0 < h, w, gs <= 16384, 0 < ratio <= 1 and a resized image of at least one pixel");
  tta_axis(w, sw, wp, flip_lr != 0, tab);
  tta_axis(h, sh, hp, 0, tab + 4 * wp);
  return HM_OK;
}

extern "C" int hm_tta_scale(const void* x, void* y, const int32_t* tab_dev, int nb, int h, int w, double ratio, int gs, int dtype,
                            void* stream_) {
  if (!x || !y || !tab_dev) return hm_set_error(HM_ERR_ARG, "hm_tta_scale: null pointer");
  if (nb <= 0 || nb > 65535) return hm_set_error(HM_ERR_ARG, "hm_tta_scale: need 0 < nb <= 65535");
  int sh, sw, hp, wp;
  if (!tta_sizes(h, w, ratio, gs, &sh, &sw, &hp, &wp))
    return hm_set_error(HM_ERR_ARG, "hm_tta_scale: need 0 < h, w, gs <= 16384, 0 < ratio <= 1 and a resized image of at least one pixel");
  if (dtype != HM_DTYPE_BF16 && dtype != HM_DTYPE_F16 && dtype != HM_DTYPE_F32) return hm_set_error(HM_ERR_ARG, "hm_tta_scale: bad dtype");
  const uintptr_t mask = dtype == HM_DTYPE_F32 ? 31 : 15;              // one pixel: 8 elements, one store
  if ((((uintptr_t)x | (uintptr_t)y) & mask) || ((uintptr_t)tab_dev & 3))
    return hm_set_error(HM_ERR_ARG, "hm_tta_scale: x and y must be aligned to a pixel (16 bytes, 32 in fp32), the table to 4 bytes");
  const int total = hp * wp;
  hipStream_t s = (hipStream_t)stream_;
  HmProfScope prof(HM_K_OTHER, 7, hp, wp, nb, s);
  const int rc = with_dtype_or_f32(dtype, [&](auto* tag) {
    using E = std::remove_pointer_t<decltype(tag)>;
    hipLaunchKernelGGL(tta_scale_kernel<E>, dim3((total + 255) / 256, nb), dim3(256), 0, s, (const E*)x, (E*)y, tab_dev, h, w, hp, wp);
    return HM_OK;
  });
  return rc != HM_OK ? rc : hm_check_launch("hm_tta_scale");
}

extern "C" int hm_yolo_decode_batch_tta(const float* raw, int ldraw, float* pred, int row0, int ny, int nx, int nc, float stride,
                                        const float* a, int nb, size_t pred_rows_per_image, float scale, int flip_lr, float full_w,
                                        void* stream_) {
  if (!raw || !pred || !a || ny <= 0 || nx <= 0 || nc <= 0 || row0 < 0 || nb <= 0 || nb > 65535)
    return hm_set_error(HM_ERR_ARG, "hm_yolo_decode_batch_tta: bad arguments");
  if (ldraw < 3 * (5 + nc)) return hm_set_error(HM_ERR_ARG, "hm_yolo_decode_batch_tta: ldraw too small");
  if (!(scale > 0.0f) || !(scale <= 1.0f)) return hm_set_error(HM_ERR_ARG, "hm_yolo_decode_batch_tta: need 0 < scale <= 1");
  if (flip_lr && !(full_w > 0.0f)) return hm_set_error(HM_ERR_ARG, "hm_yolo_decode_batch_tta: a flipped pass needs the full width");
  hipStream_t s = (hipStream_t)stream_;
  HmProfScope prof(HM_K_OTHER, 4, ny, nx, nc, s);
  hipLaunchKernelGGL(decode_tta_kernel, dim3((3 * ny * nx + 255) / 256, nb), dim3(256), 0, s, raw, ldraw, pred, row0, ny, nx, 5 + nc,
                     stride, a[0], a[1], a[2], a[3], a[4], a[5], (size_t)ny * nx * ldraw, pred_rows_per_image * (5 + nc), scale,
                     flip_lr != 0, full_w);
  return hm_check_launch("hm_yolo_decode_batch_tta");
}
