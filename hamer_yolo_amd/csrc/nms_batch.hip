// non_max_suppression (utils/general.py:611-703, labels=(), merge=False) for every image of a pass in one call:
//   one memset of the per-image counters, one filter launch over nb * n rows, one suppression launch of nb workgroups.
// Both branches of the reference: best class per row (:665-667) and multi-label (:662-664, one candidate per (row, class)).
// The arithmetic is hm_yolo_nms's (yolo.hip), expression for expression, so best-class results are the same bytes.
//
// A candidate is its 64-bit sort key alone: (sortable(score) << 32) | ~(row * nc + class).  Score and class come back out of
// the key, the box is one float4 per ROW (x1, y1, x2, y2 without class offset), so multi-label costs 8 bytes per candidate.
// Descending key order = descending score, equal scores by ascending (row, class): the stable order of the reference's
// row-major nonzero().  In best-class mode a row has one candidate and this is hm_yolo_nms's order by row.
//
// Workspace of hm_nms_batch_workspace_bytes(nb, n, nc, multi_label), with C = n * (multi_label && nc > 1 ? nc : 1):
//   [0, A)                       int counter[nb], A = nb * 4 rounded up to 256
//   then per image, S bytes each: u64 keys[pow2(C)] | float4 box[n] | float4 sorted[min(C, 30000)]
//   S = pow2(C) * 8 + n * 16 + min(C, 30000) * 16          total = A + nb * S
// `sorted` holds the boxes plus class offset in suppression order, so the sweeps read consecutive float4s and not key -> row
// -> box; the first 1024 of them live in LDS only.
#include <math.h>
#include <string.h>
#include "common.h"
#include "hamer_hip_internal.h"

namespace {

constexpr int NB_LDS_KEYS = 16384;   // keys sorted in LDS at once
constexpr int NB_MAX_NMS = 30000;    // general.py:625
constexpr int NB_MAX_CAND = 1 << 20;
constexpr int NB_BOXCACHE = 1024;
constexpr int NB_SUPP_WORDS = 1024;  // 32768 bits >= NB_MAX_NMS
constexpr int NB_LDS = NB_LDS_KEYS * 8 + NB_BOXCACHE * 16 + NB_SUPP_WORDS * 4 + 16 + 4096;
typedef unsigned long long u64;

__host__ __device__ inline int nb_pow2(int n) { int p = 1; while (p < n) p <<= 1; return p; }
__host__ __device__ inline size_t nb_image_bytes(int n, int cand) {
  return (size_t)nb_pow2(cand) * 8 + (size_t)n * 16 + (size_t)(cand < NB_MAX_NMS ? cand : NB_MAX_NMS) * 16;
}
inline size_t nb_counter_bytes(int nb) { return ((size_t)nb * 4 + 255) / 256 * 256; }

__device__ __forceinline__ unsigned nb_sortable(float f) {
  const unsigned u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float nb_unsortable(unsigned s) { return __uint_as_float((s & 0x80000000u) ? (s ^ 0x80000000u) : ~s); }

// grid (ceil(n / 256), nb): a wave never spans two images, so one atomicAdd per wave and class reserves the wave's slots
__global__ __launch_bounds__(256) void nmsb_filter_kernel(const float* __restrict__ pred, size_t pred_stride, int n, int nc,
                                                          int multi, float conf_thres, unsigned class_mask, char* __restrict__ ws,
                                                          size_t ws_counters, size_t ws_image, size_t ws_keys_bytes) {
  const int img = blockIdx.y;
  const int i = blockIdx.x * 256 + threadIdx.x;
  int* counter = (int*)ws + img;
  u64* keys = (u64*)(ws + ws_counters + (size_t)img * ws_image);
  float4* box = (float4*)(ws + ws_counters + (size_t)img * ws_image + ws_keys_bytes);
  const float* p = pred + (size_t)img * pred_stride + (size_t)(i < n ? i : 0) * (5 + nc);
  const float obj = p[4];
  const bool live = i < n && obj > conf_thres;                         // xc = prediction[..., 4] > conf_thres
  if (live) {
    const float hw = p[2] / 2, hh = p[3] / 2;                          // xywh2xyxy (general.py:268-275)
    box[i] = make_float4(p[0] - hw, p[1] - hh, p[0] + hw, p[1] + hh);
  }
  const unsigned lane = threadIdx.x & 63;
  auto append = [&](bool take, float s, int c) {                       // wave-uniform call
    const u64 m = __ballot(take);
    if (!m) return;
    int base = 0;
    if (lane == (unsigned)(__ffsll((long long)m) - 1)) base = atomicAdd(counter, __popcll(m));
    base = __shfl(base, __ffsll((long long)m) - 1);
    if (take) keys[base + __popcll(m & ((1ull << lane) - 1ull))] = ((u64)nb_sortable(s) << 32) | (0xFFFFFFFFu - (unsigned)(i * nc + c));
  };
  if (multi) {                                                         // (x[:, 5:] > conf_thres).nonzero(): every class above it
    for (int c = 0; c < nc; ++c) {
      const float s = live ? __fmul_rn(p[5 + c], obj) : 0.0f;           // x[:, 5:] *= x[:, 4:5]
      append(live && s > conf_thres && ((class_mask >> c) & 1u), s, c);
    }
  } else {
    float best = -1.0f; int bj = 0;
    if (live)
      for (int c = 0; c < nc; ++c) {
        const float s = nc == 1 ? obj : __fmul_rn(p[5 + c], obj);
        if (s > best) { best = s; bj = c; }                            // first maximum, as torch.max
      }
    append(live && best > conf_thres && ((class_mask >> bj) & 1u), best, bj);
  }
}

__device__ __forceinline__ void nmsb_cx(u64* a, int j, int l, bool desc) {
  const u64 x = a[j], y = a[l];
  if (desc ? (x < y) : (x > y)) { a[j] = y; a[l] = x; }
}

// the bitonic stages k0..k1 (strides below cnt) on the cnt keys of `a`, which are keys base.. of the whole sequence
__device__ void nmsb_stages(u64* a, int cnt, int base, int k0, int k1, int tid) {
  for (int k = k0; k <= k1; k <<= 1)
    for (int s = (k >> 1) < (cnt >> 1) ? (k >> 1) : (cnt >> 1); s > 0; s >>= 1) {
      for (int j = tid; j < cnt; j += 1024) {
        const int l = j ^ s;
        if (l > j) nmsb_cx(a, j, l, ((base + j) & k) == 0);
      }
      __syncthreads();
    }
}

__global__ __launch_bounds__(1024) void nmsb_kernel(char* __restrict__ ws, size_t ws_counters, size_t ws_image, size_t ws_keys_bytes,
                                                    int n_rows, int nc, float iou_thres, int agnostic, int max_det,
                                                    hm_letterbox_plan pl, int do_scale, float* __restrict__ dets_all,
                                                    size_t dets_stride, int* __restrict__ count_all) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  u64* lkeys = (u64*)smem;                                                          // NB_LDS_KEYS
  float4* bcache = (float4*)(smem + NB_LDS_KEYS * 8);                               // NB_BOXCACHE
  unsigned* supp = (unsigned*)(smem + NB_LDS_KEYS * 8 + NB_BOXCACHE * 16);          // NB_SUPP_WORDS
  int* kept = (int*)(smem + NB_LDS_KEYS * 8 + NB_BOXCACHE * 16 + NB_SUPP_WORDS * 4 + 16);   // <= 1024 entries
  const int tid = threadIdx.x, img = blockIdx.x;
  char* mine = ws + ws_counters + (size_t)img * ws_image;
  u64* gkeys = (u64*)mine;
  const float4* box = (const float4*)(mine + ws_keys_bytes);
  float4* sorted = (float4*)(mine + ws_keys_bytes + (size_t)n_rows * 16);
  float* dets = dets_all + (size_t)img * dets_stride * 6;
  int n = ((const int*)ws)[img];
  const int P = nb_pow2(n);
  const bool in_lds = n <= NB_LDS_KEYS;
  for (int j = tid; j < NB_SUPP_WORDS; j += 1024) supp[j] = 0u;
  // descending bitonic sort (a real key has its top bit set: scores are > conf_thres >= 0, so the zero padding sorts last)
  if (in_lds) {
    for (int j = tid; j < P; j += 1024) lkeys[j] = j < n ? gkeys[j] : 0ull;
    __syncthreads();
    nmsb_stages(lkeys, P, 0, 2, P, tid);
  } else {
    // more keys than LDS holds: strides below NB_LDS_KEYS run on one LDS-sized chunk at a time, the others in the workspace
    auto chunks = [&](int k0, int k1) {
      for (int base = 0; base < P; base += NB_LDS_KEYS) {
        for (int j = tid; j < NB_LDS_KEYS; j += 1024) lkeys[j] = base + j < n || k0 > 2 ? gkeys[base + j] : 0ull;
        __syncthreads();
        nmsb_stages(lkeys, NB_LDS_KEYS, base, k0, k1, tid);
        for (int j = tid; j < NB_LDS_KEYS; j += 1024) gkeys[base + j] = lkeys[j];
        __syncthreads();
      }
    };
    chunks(2, NB_LDS_KEYS);                                                         // also writes the zero padding up to P
    for (int k = 2 * NB_LDS_KEYS; k <= P; k <<= 1) {
      for (int s = k >> 1; s >= NB_LDS_KEYS; s >>= 1) {
        for (int j = tid; j < P; j += 1024) {
          const int l = j ^ s;
          if (l > j) nmsb_cx(gkeys, j, l, (j & k) == 0);
        }
        __syncthreads();
      }
      chunks(k, k);
    }
  }
  const u64* keys = in_lds ? lkeys : gkeys;
  n = n < NB_MAX_NMS ? n : NB_MAX_NMS;                                          // x[x[:, 4].argsort(descending=True)[:max_nms]]
  const float off = agnostic ? 0.0f : 4096.0f;                                 // c = cls * max_wh (general.py:685)
  auto index_of = [&](int j) { return 0xFFFFFFFFu - (unsigned)(keys[j] & 0xFFFFFFFFull); };
  for (int j = tid; j < n; j += 1024) {
    const unsigned idx = index_of(j);
    const float4 b = box[idx / (unsigned)nc];
    const float o = (float)(idx % (unsigned)nc) * off;
    const float4 v = make_float4(b.x + o, b.y + o, b.z + o, b.w + o);          // x[:, :4] + c, rounded to fp32
    if (j < NB_BOXCACHE) bcache[j] = v; else sorted[j] = v;
  }
  __syncthreads();
  int nk = 0;
  for (int i = 0; i < n && nk < max_det; ++i) {
    if ((supp[i >> 5] >> (i & 31)) & 1u) continue;                            // uniform: read after a barrier
    if (tid == 0) kept[nk] = i;
    ++nk;
    const float4 bi = i < NB_BOXCACHE ? bcache[i] : sorted[i];
    const float iarea = __fmul_rn(bi.z - bi.x, bi.w - bi.y);
    for (int j = i + 1 + tid; j < n; j += 1024) {
      if ((supp[j >> 5] >> (j & 31)) & 1u) continue;
      const float4 bj = j < NB_BOXCACHE ? bcache[j] : sorted[j];
      const float w = fmaxf(0.0f, fminf(bi.z, bj.z) - fmaxf(bi.x, bj.x));
      const float h = fmaxf(0.0f, fminf(bi.w, bj.w) - fmaxf(bi.y, bj.y));
      const float inter = __fmul_rn(w, h);
      const float jarea = __fmul_rn(bj.z - bj.x, bj.w - bj.y);
      const float ovr = inter / (__fadd_rn(iarea, jarea) - inter);
      if (ovr > iou_thres) atomicOr(&supp[j >> 5], 1u << (j & 31));
    }
    __syncthreads();
  }
  __syncthreads();
  if (tid == 0) count_all[img] = nk;
  for (int r = tid; r < nk; r += 1024) {
    const u64 key = keys[kept[r]];
    const unsigned idx = 0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull);
    const float4 c = box[idx / (unsigned)nc];
    float b[4] = {c.x, c.y, c.z, c.w};
    if (do_scale) {                                                            // scale_coords + clip + round
      const float lim[4] = {(float)pl.src_w, (float)pl.src_h, (float)pl.src_w, (float)pl.src_h};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float t = (b[e] - ((e & 1) ? pl.pad_y : pl.pad_x)) / pl.gain;
        t = fminf(fmaxf(t, 0.0f), lim[e]);
        b[e] = rintf(t);
      }
    }
    float* o = dets + (size_t)r * 6;
    o[0] = b[0]; o[1] = b[1]; o[2] = b[2]; o[3] = b[3]; o[4] = nb_unsortable((unsigned)(key >> 32)); o[5] = (float)(idx % (unsigned)nc);
  }
}

inline int nb_cand(int n, int nc, int multi_label) { return (multi_label && nc > 1) ? n * nc : n; }
inline bool nb_shape_ok(int nb, int n, int nc, int multi_label) {
  if (nb < 1 || nb > 4096 || nc <= 0 || nc > 32 || n <= 0 || n > NB_MAX_CAND) return false;
  return (long long)n * ((multi_label && nc > 1) ? nc : 1) <= NB_MAX_CAND;
}

}  // namespace

extern "C" size_t hm_nms_batch_workspace_bytes(int nb, int n, int nc, int multi_label) {
  if (!nb_shape_ok(nb, n, nc, multi_label)) return 0;
  return nb_counter_bytes(nb) + (size_t)nb * nb_image_bytes(n, nb_cand(n, nc, multi_label));
}

extern "C" int hm_yolo_nms_batch(const float* pred, size_t pred_image_stride, int nb, int n, int nc, float conf_thres,
                                 float iou_thres, unsigned class_mask, int agnostic, int multi_label, int max_det,
                                 const hm_letterbox_plan* plan, float* dets, size_t dets_image_stride, int* count, void* workspace,
                                 size_t workspace_bytes, void* stream_) {
  if (!pred || !dets || !count || !workspace) return hm_set_error(HM_ERR_ARG, "hm_yolo_nms_batch: null pointer");
  if (nb < 1 || nb > 4096) return hm_set_error(HM_ERR_ARG, "hm_yolo_nms_batch: need 1 <= nb <= 4096");
  if (nc <= 0 || nc > 32 || max_det <= 0 || max_det > 1024)
    return hm_set_error(HM_ERR_ARG, "hm_yolo_nms_batch: need 0 < nc <= 32, 0 < max_det <= 1024");
  multi_label = (multi_label && nc > 1) ? 1 : 0;                       // multi_label &= nc > 1 (general.py:628)
  if (!nb_shape_ok(nb, n, nc, multi_label))
    return hm_set_error(HM_ERR_ARG, "hm_yolo_nms_batch: need n > 0 and n * (multi_label ? nc : 1) <= 1048576");
  if (!(conf_thres >= 0.0f)) return hm_set_error(HM_ERR_ARG, "hm_yolo_nms_batch: conf_thres must be >= 0");
  if (dets_image_stride < (size_t)max_det) return hm_set_error(HM_ERR_ARG, "hm_yolo_nms_batch: dets_image_stride smaller than max_det");
  if (workspace_bytes < hm_nms_batch_workspace_bytes(nb, n, nc, multi_label) || ((uintptr_t)workspace & 15))
    return hm_set_error(HM_ERR_ARG, "hm_yolo_nms_batch: workspace too small or misaligned");
  hipStream_t s = (hipStream_t)stream_;
  static HmLdsOnce lds_once;
  if (const int rc = lds_once.ensure((const void*)nmsb_kernel, NB_LDS, "hm_yolo_nms_batch: cannot raise dynamic LDS limit")) return rc;
  const int cand = nb_cand(n, nc, multi_label);
  const size_t counters = nb_counter_bytes(nb), image = nb_image_bytes(n, cand), keys_bytes = (size_t)nb_pow2(cand) * 8;
  if (hipMemsetAsync(workspace, 0, counters, s) != hipSuccess) return hm_set_error(HM_ERR_HIP, "hm_yolo_nms_batch: memset failed");
  HmProfScope prof(HM_K_OTHER, 5, n, nc, nb, s);
  hipLaunchKernelGGL(nmsb_filter_kernel, dim3((n + 255) / 256, nb), dim3(256), 0, s, pred, pred_image_stride, n, nc, multi_label,
                     conf_thres, class_mask, (char*)workspace, counters, image, keys_bytes);
  hm_letterbox_plan pl;
  memset(&pl, 0, sizeof(pl));
  if (plan) pl = *plan;
  hipLaunchKernelGGL(nmsb_kernel, dim3(nb), dim3(1024), NB_LDS, s, (char*)workspace, counters, image, keys_bytes, n, nc, iou_thres,
                     agnostic, max_det, pl, plan ? 1 : 0, dets, dets_image_stride, count);
  return hm_check_launch("hm_yolo_nms_batch");
}
