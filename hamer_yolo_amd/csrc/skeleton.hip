// Hand skeletons drawn onto images (reference: rootnet/vis_tool.py draw_2d_skeleton, :602-640; hamer/utils/draw_2d_skeleton.py;
// hamer/utils/render_openpose.py render_keypoints, :56-91): 20 bones and 21 joint discs per hand, opaque, for a batch of
// equally sized images.  The drawing rule is stated in include/hamer_hip.h (hm_skeleton_overlay) and DESIGN.md section 8.2;
// tests/skeleton_rule.py restates it in numpy as a sequential painter.  Here it is evaluated per pixel:
//  * setup  - one wave per hand: the 21 integer points and which are absent, per bone the fp64 step 1.0 / m (one IEEE
//             division), the hand's box (its present points grown by the larger radius, clipped to the image); every 16 x 16
//             tile of the box is claimed once per image through a flag byte and appended to a work list through one atomic
//             counter (no host readback of any box).
//  * raster - a grid-strided loop over the work list, one workgroup (4 waves) per tile, one lane per pixel: the hands of the
//             tile's image whose box meets the tile are gathered into LDS in table order (ballot + prefix), and each lane walks
//             hands and primitives from last to first and stops at the first cover, so a pixel gets the covering primitive of
//             largest (hand, draw index) whatever the order of the work list.  Only covered pixels are written.
// The host sorts the hand table by image (stable, so table order survives inside an image) and hands each image's range of
// hands to the kernels, so a tile looks at its own image's hands only.  The copying form is one device-to-device copy
// followed by the in-place form on `out`.
// On the major axis of a bone (|d| == m) the rule's sample rint(a + t_i*d) is a + sign(d)*i exactly: t_i*d differs from
// sign(d)*i by less than i * 2^-51 <= 2^-35 (|d| < 2^16: two roundings of relative size 2^-53 each), nowhere near a tie.  So
// a pixel at signed major-axis offset c from `a` can only be covered by the samples c - r .. c + r, and only their minor
// coordinate needs the fp64 expression, evaluated without contraction as numpy does.
#include <math.h>
#include "common.h"
#include "raster_tiles.h"

namespace {
using namespace raster_tiles;

constexpr int NJ = 21;
constexpr int MAX_RADIUS = 32, MAX_SIDE = 16384;
constexpr int HANDS_PER_LAUNCH = 128;              // setup kernel argument block stays under 4 KiB
constexpr int CHUNK = 64;                          // hands gathered into LDS at a time

struct HandArg {
  int image, line_radius, joint_radius;
  float threshold;
  int row;                                         // the hand's row in kp
  int first, count;                                // the image's hands: sorted positions first .. first + count - 1
};
struct HandBlock {
  HandArg h[HANDS_PER_LAUNCH];
  int count, first;                                // sorted positions first .. first + count - 1 of the call
};
struct Palette { unsigned c[NJ]; };                 // byte k of c[j] goes to channel k

// Per hand, written by setup, indexed by the sorted position.
struct HandRec {
  double step[NJ];                                 // step[j] = 1.0 / m of bone j (j >= 1, m > 0)
  int px[NJ], py[NJ];
  unsigned present;                                // bit j: joint j is drawn
  int line_radius, joint_radius;
  int bx0, by0, bx1, by1;                          // clipped box, empty when bx0 > bx1
  int pad;
};
static_assert(sizeof(HandRec) % 8 == 0, "HandRec is copied as 8-byte words");

struct Layout { size_t counter, flags, ranges, items, recs, total; };

Layout layout(int N, int H, int W, int n_hands) {
  const size_t tiles = tiles_of(H, W);
  Layout L;
  L.counter = 0;
  L.flags = 256;                                                       // one byte per (image, tile): the tile is on the list
  L.ranges = align256(L.flags + (size_t)N * tiles);                    // int2 per image: its hands
  L.items = align256(L.ranges + (size_t)N * sizeof(int2));
  L.recs = align256(L.items + (size_t)N * tiles * sizeof(int2));       // a tile is listed at most once
  L.total = align256(L.recs + (size_t)n_hands * sizeof(HandRec));
  return L;
}

__device__ __forceinline__ int parent_of(int j) { return j % 4 == 1 ? 0 : j - 1; }

// One wave per hand of the block.
__global__ __launch_bounds__(64) void skeleton_setup_kernel(HandBlock hb, const float* __restrict__ kp, int kp_stride, int H, int W,
                                                            char* __restrict__ ws, Layout L) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x;
  const HandArg a = hb.h[blockIdx.x];
  const int pos = hb.first + blockIdx.x;
  __shared__ HandRec rec;
  __shared__ int bx0, by0, bx1, by1;
  if (lane == 0) { bx0 = INT_MAX; by0 = INT_MAX; bx1 = INT_MIN; by1 = INT_MIN; rec.present = 0u; }
  __syncthreads();
  if (lane < NJ) {
    const float* p = kp + ((size_t)a.row * NJ + lane) * kp_stride;
    const float u = p[0], v = p[1];
    bool ok = fabsf(u) < 32768.0f && fabsf(v) < 32768.0f;             // false for NaN and inf
    if (kp_stride == 3) ok = ok && p[2] > a.threshold;
    const int x = ok ? (int)u : 0, y = ok ? (int)v : 0;               // truncation toward zero
    rec.px[lane] = x; rec.py[lane] = y;
    if (ok) {
      atomicOr(&rec.present, 1u << lane);
      atomicMin(&bx0, x); atomicMin(&by0, y); atomicMax(&bx1, x); atomicMax(&by1, y);
    }
  }
  __syncthreads();
  if (lane < NJ) {
    double step = 0.0;
    if (lane > 0) {
      const int q = parent_of(lane);
      const int dx = rec.px[lane] - rec.px[q], dy = rec.py[lane] - rec.py[q];
      const int m = max(abs(dx), abs(dy));
      if (m > 0) step = 1.0 / (double)m;
    }
    rec.step[lane] = step;
  }
  const int grow = max(a.line_radius, a.joint_radius);
  int cx0 = 1, cy0 = 1, cx1 = 0, cy1 = 0;                              // empty
  if (bx0 <= bx1) { cx0 = max(bx0 - grow, 0); cy0 = max(by0 - grow, 0); cx1 = min(bx1 + grow, W - 1); cy1 = min(by1 + grow, H - 1); }
  const bool any = cx0 <= cx1 && cy0 <= cy1;
  if (lane == 0) {
    rec.line_radius = a.line_radius; rec.joint_radius = a.joint_radius;
    rec.bx0 = any ? cx0 : 1; rec.by0 = any ? cy0 : 1; rec.bx1 = any ? cx1 : 0; rec.by1 = any ? cy1 : 0;
    rec.pad = 0;
    ((int2*)(ws + L.ranges))[a.image] = make_int2(a.first, a.count);   // every hand of an image writes the same pair
  }
  __syncthreads();
  const unsigned long long* src = (const unsigned long long*)&rec;
  unsigned long long* dst = (unsigned long long*)(ws + L.recs + (size_t)pos * sizeof(HandRec));
  for (int i = lane; i < (int)(sizeof(HandRec) / 8); i += 64) dst[i] = src[i];
  if (!any) return;
  const int tiles_x = (W + TILE - 1) / TILE, tiles = tiles_x * ((H + TILE - 1) / TILE);
  const int tx0 = cx0 / TILE, ty0 = cy0 / TILE, ntx = cx1 / TILE - tx0 + 1, nty = cy1 / TILE - ty0 + 1;
  unsigned* flags = (unsigned*)(ws + L.flags);                          // bytes, claimed through their aligned word
  int2* items = (int2*)(ws + L.items);
  for (int t = lane; t < ntx * nty; t += 64) {
    const int tx = tx0 + t % ntx, ty = ty0 + t / ntx;
    const size_t f = (size_t)a.image * tiles + (size_t)ty * tiles_x + tx;
    const unsigned bit = 1u << (8 * (f & 3));
    if (!(atomicOr(flags + (f >> 2), bit) & bit)) {
      const unsigned slot = atomicAdd((unsigned*)(ws + L.counter), 1u);
      items[slot] = make_int2(a.image, pack_tile(tx, ty));
    }
  }
}

__device__ __forceinline__ bool in_disc(int x, int y, int cx, int cy, int r) {
  const int dx = x - cx, dy = y - cy;
  if (dx > r || dx < -r || dy > r || dy < -r) return false;            // also keeps the squares small
  return dx * dx + dy * dy <= r * r;
}

// Does bone a -> b (step = 1.0 / m) of radius r cover pixel (x, y)?
__device__ __forceinline__ bool in_bone(int x, int y, int ax, int ay, int bx, int by, double step, int r) {
#pragma clang fp contract(off)
  if (x < min(ax, bx) - r || x > max(ax, bx) + r || y < min(ay, by) - r || y > max(ay, by) + r) return false;
  const int dx = bx - ax, dy = by - ay;
  const int m = max(abs(dx), abs(dy));
  if (m == 0) return in_disc(x, y, ax, ay, r);
  const bool xmajor = abs(dx) >= abs(dy);
  const int amaj = xmajor ? ax : ay, amin = xmajor ? ay : ax;
  const int dmaj = xmajor ? dx : dy, dmin = xmajor ? dy : dx;
  const int pmaj = xmajor ? x : y, pmin = xmajor ? y : x;
  const int sgn = dmaj > 0 ? 1 : -1;
  const int c = (pmaj - amaj) * sgn;
  const int i0 = max(c - r, 0), i1 = min(c + r, m);
  for (int i = i0; i <= i1; ++i) {
    const double t = i < m ? (double)i * step : 1.0;
    const int smin = (int)rint((double)amin + t * (double)dmin);
    const int e = c - i, f = pmin - smin;
    if (f <= r && f >= -r && e * e + f * f <= r * r) return true;
  }
  return false;
}

// The joint whose colour hand h gives pixel (x, y), or -1.
__device__ __forceinline__ int hand_cover(const HandRec& h, int x, int y, int order) {
  if (x < h.bx0 || x > h.bx1 || y < h.by0 || y > h.by1) return -1;
  const unsigned present = h.present;
  const int lr = h.line_radius, jr = h.joint_radius;
  if (order == HM_SKEL_BONES_FIRST) {
    for (int j = NJ - 1; j >= 0; --j)
      if ((present >> j & 1u) && in_disc(x, y, h.px[j], h.py[j], jr)) return j;
    for (int j = NJ - 1; j >= 1; --j) {
      const int q = parent_of(j);
      if ((present >> j & 1u) && (present >> q & 1u) && in_bone(x, y, h.px[q], h.py[q], h.px[j], h.py[j], h.step[j], lr)) return j;
    }
    return -1;
  }
  for (int j = NJ - 1; j >= 0; --j) {
    if (!(present >> j & 1u)) continue;
    if (in_disc(x, y, h.px[j], h.py[j], jr)) return j;
    if (j == 0) break;
    const int q = parent_of(j);
    if ((present >> q & 1u) && in_bone(x, y, h.px[q], h.py[q], h.px[j], h.py[j], h.step[j], lr)) return j;
  }
  return -1;
}

// Grid-strided over the work list; one lane per pixel of a 16 x 16 tile.
__global__ __launch_bounds__(256) void skeleton_raster_kernel(uint8_t* __restrict__ out, int H, int W, Palette pal, int order,
                                                              const char* __restrict__ ws, Layout L) {
  __shared__ HandRec s_hand[CHUNK];
  __shared__ unsigned s_pal[NJ];
  __shared__ int s_src[CHUNK], s_n;
  const int tid = threadIdx.x;
  if (tid < NJ) s_pal[tid] = pal.c[tid];                               // visible after the first barrier below
  const unsigned count = *(const unsigned*)(ws + L.counter);
  const int2* items = (const int2*)(ws + L.items);
  const int2* ranges = (const int2*)(ws + L.ranges);
  const HandRec* recs = (const HandRec*)(ws + L.recs);
  for (unsigned w = blockIdx.x; w < count; w += gridDim.x) {
    const int2 it = items[w];
    const int2 range = ranges[it.x];
    const int x0 = tile_x(it.y) * TILE, y0 = tile_y(it.y) * TILE;
    const int px = x0 + (tid & (TILE - 1)), py = y0 + (tid >> 4);
    int joint = -1;
    for (int c0 = 0; c0 < range.y; c0 += CHUNK) {
      // the first wave culls CHUNK hands against the tile; their records go to LDS in table order
      if (tid < 64) {
        const int k = c0 + tid;
        bool hit = false;
        if (k < range.y) {
          const HandRec& r = recs[range.x + k];
          hit = box_meets_tile(make_int4(r.bx0, r.by0, r.bx1, r.by1), x0, y0);
        }
        const unsigned long long mask = __ballot(hit);
        if (hit) {
          const int slot = __popcll(mask & ((1ull << tid) - 1));
          s_src[slot] = k;
        }
        if (tid == 0) s_n = __popcll(mask);
      }
      __syncthreads();
      const int n = s_n;
      constexpr int WORDS = sizeof(HandRec) / 8;
      for (int i = tid; i < n * WORDS; i += 256)
        ((unsigned long long*)s_hand)[i] = ((const unsigned long long*)(recs + range.x + s_src[i / WORDS]))[i % WORDS];
      __syncthreads();
      if (px < W && py < H) {
        for (int q = n - 1; q >= 0; --q) {
          const int j = hand_cover(s_hand[q], px, py, order);
          if (j >= 0) { joint = j; break; }                           // a later chunk's hands go over this one's
        }
      }
      __syncthreads();                                                 // the list is rewritten by the next chunk
    }
    if (joint >= 0) {
      uint8_t* dst = out + (((size_t)it.x * H + py) * W + px) * 3;
      const unsigned c = s_pal[joint];
      dst[0] = (uint8_t)c; dst[1] = (uint8_t)(c >> 8); dst[2] = (uint8_t)(c >> 16);
    }
  }
}

int check_args(const uint8_t* images, int N, int H, int W, const float* kp, int kp_stride, const hm_skeleton* hands, int n_hands,
               const uint8_t* palette, int order, const uint8_t* out, const void* ws, size_t ws_bytes) {
  if (N <= 0 || H <= 0 || W <= 0 || H > MAX_SIDE || W > MAX_SIDE)
    return hm_set_error(HM_ERR_ARG, "hm_skeleton_overlay: need N >= 1 and 1 <= H, W <= 16384");
  if (kp_stride != 2 && kp_stride != 3) return hm_set_error(HM_ERR_ARG, "hm_skeleton_overlay: kp_stride must be 2 or 3");
  if (order != HM_SKEL_INTERLEAVED && order != HM_SKEL_BONES_FIRST) return hm_set_error(HM_ERR_ARG, "hm_skeleton_overlay: unknown order");
  if (n_hands < 0) return hm_set_error(HM_ERR_ARG, "hm_skeleton_overlay: negative hand count");
  if (!images || !out) return hm_set_error(HM_ERR_ARG, "hm_skeleton_overlay: null images or out");
  if (n_hands > 0 && (!kp || !hands || !palette || !ws)) return hm_set_error(HM_ERR_ARG, "hm_skeleton_overlay: null pointer with hands to draw");
  const size_t fb = (size_t)N * H * W * 3;
  if (out != images && images < out + fb && out < images + fb)
    return hm_set_error(HM_ERR_ARG, "hm_skeleton_overlay: out partly overlaps images (equal or disjoint)");
  for (int i = 0; i < n_hands; ++i) {
    const hm_skeleton& h = hands[i];
    if (h.image < 0 || h.image >= N) return hm_set_error(HM_ERR_ARG, "hm_skeleton_overlay: hand image outside the batch");
    if (h.line_radius < 0 || h.line_radius > MAX_RADIUS || h.joint_radius < 0 || h.joint_radius > MAX_RADIUS)
      return hm_set_error(HM_ERR_ARG, "hm_skeleton_overlay: radius outside 0..32");
  }
  if (n_hands > 0 && ws_bytes < layout(N, H, W, n_hands).total) return hm_set_error(HM_ERR_ARG, "hm_skeleton_overlay: workspace too small");
  return HM_OK;
}

}  // namespace

extern "C" size_t hm_skeleton_overlay_workspace_bytes(int N, int H, int W, int n_hands) {
  if (N <= 0 || H <= 0 || W <= 0 || H > MAX_SIDE || W > MAX_SIDE || n_hands <= 0) return 0;
  return layout(N, H, W, n_hands).total;
}

extern "C" int hm_skeleton_overlay(const uint8_t* images, int N, int H, int W, const float* kp, int kp_stride,
                                   const hm_skeleton* hands_host, int n_hands, const uint8_t* palette_host, int order, uint8_t* out,
                                   void* workspace, size_t workspace_bytes, void* stream_) {
  const int rc = check_args(images, N, H, W, kp, kp_stride, hands_host, n_hands, palette_host, order, out, workspace, workspace_bytes);
  if (rc != HM_OK) return rc;
  hipStream_t s = (hipStream_t)stream_;
  HmProfScope prof(HM_K_OTHER, 0, N, H, W, s);
  if (out != images &&
      hipMemcpyAsync(out, images, (size_t)N * H * W * 3, hipMemcpyDeviceToDevice, s) != hipSuccess)
    return hm_set_error(HM_ERR_HIP, "hm_skeleton_overlay: hipMemcpyAsync");
  if (n_hands == 0) return HM_OK;
  const Layout L = layout(N, H, W, n_hands);
  char* ws = (char*)workspace;
  if (hipMemsetAsync(ws + L.counter, 0, L.ranges - L.counter, s) != hipSuccess)          // counter and tile flags
    return hm_set_error(HM_ERR_HIP, "hm_skeleton_overlay: hipMemsetAsync");
  // table order inside an image is the drawing order: a stable sort by image keeps it
  std::vector<int> rows(n_hands);
  std::iota(rows.begin(), rows.end(), 0);
  std::stable_sort(rows.begin(), rows.end(), [&](int a, int b) { return hands_host[a].image < hands_host[b].image; });
  std::vector<int> first(n_hands), count(n_hands);
  for (int i = 0, j; i < n_hands; i = j) {
    for (j = i; j < n_hands && hands_host[rows[j]].image == hands_host[rows[i]].image; ++j) {}
    for (int k = i; k < j; ++k) { first[k] = i; count[k] = j - i; }
  }
  for (int b0 = 0; b0 < n_hands; b0 += HANDS_PER_LAUNCH) {
    HandBlock hb;
    hb.first = b0;
    hb.count = n_hands - b0 < HANDS_PER_LAUNCH ? n_hands - b0 : HANDS_PER_LAUNCH;
    for (int i = 0; i < hb.count; ++i) {
      const hm_skeleton& h = hands_host[rows[b0 + i]];
      hb.h[i] = HandArg{h.image, h.line_radius, h.joint_radius, h.threshold, rows[b0 + i], first[b0 + i], count[b0 + i]};
    }
    hipLaunchKernelGGL(skeleton_setup_kernel, dim3(hb.count), dim3(64), 0, s, hb, kp, kp_stride, H, W, ws, L);
  }
  Palette pal;
  for (int j = 0; j < NJ; ++j)
    pal.c[j] = palette_host[j * 3] | ((unsigned)palette_host[j * 3 + 1] << 8) | ((unsigned)palette_host[j * 3 + 2] << 16);
  const int grid = raster_grid(std::min((size_t)N, (size_t)n_hands), H, W, 4096);   // a hand touches tiles of one image
  hipLaunchKernelGGL(skeleton_raster_kernel, dim3(grid), dim3(256), 0, s, out, H, W, pal, order, (const char*)ws, L);
  return hm_check_launch("hm_skeleton_overlay");
}
