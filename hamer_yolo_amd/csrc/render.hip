// Mesh overlay (reference: hamer/reconstruct.py project_and_draw, :50-86): every face of every hand mesh filled into its
// frame and blended with it, for a batch of equally sized frames in three launches.  The drawing rule is stated in
// include/hamer_hip.h (hm_mesh_overlay) and DESIGN.md section 8; tests/render_rule.py restates it in numpy.
//  * setup   - one workgroup per mesh: per face the fp64 projection of its corners, the validity test, the depth key, the
//              integer bounding box clipped to the frame and the colour; the mesh's clipped box, cut into 16 x 16 tiles,
//              appended to a work list through one atomic counter (no host readback of any box).
//  * raster  - a grid-strided loop over the work list: per (mesh, tile) the mesh's faces are culled against the tile into an
//              LDS list (ballot + prefix), one lane per pixel finds the nearest covering face, and the winning 64-bit key
//              (fp32 mean depth, face id) goes into the frame's key buffer with one unsigned 64-bit atomicMin.
//  * compose - one pass over the frames: key -> face -> colour -> output frame (never in place); the key is reset on the
//              way, so the key buffer is filled once when it is allocated and stays clean between calls.
// The tile list, the cull step and the key buffer's contract are raster_tiles.h's, shared with zrender.hip.
// Every fp32 / fp64 expression of the rule is evaluated without contraction (`#pragma clang fp contract(off)`), in the
// order the rule gives, so the bytes are those of the numpy restatement.
#include <math.h>
#include "common.h"
#include "raster_tiles.h"

namespace {
using namespace raster_tiles;

constexpr int MESHES_PER_LAUNCH = 120;             // setup kernel argument block stays under 4 KiB
constexpr int F_DEGENERATE = 1, F_SMALL = 2;       // FaceRec.flags

struct MeshBlock {
  hm_mesh m[MESHES_PER_LAUNCH];
  int count, first;                                // meshes first .. first + count - 1 of the call
};

// Per face, written by setup, indexed by the global face id (the face's row in `faces`).
struct FaceRec {
  int x0, y0, x1, y1, x2, y2;                      // integer pixel corners
  unsigned depth;                                  // bits of the fp32 mean corner depth (> 0, so ordered as unsigned)
  int flags;
};

using Layout = TileLayout;                         // tail: one packed B G R colour per face
Layout layout(int N, int H, int W, int n_meshes, int n_faces) {
  return tile_layout(N, H, W, n_meshes, n_faces, sizeof(FaceRec), (size_t)n_faces * 4);
}

// Closed-triangle coverage of pixel (px, py), already known to lie inside the face's bounding box.  F_SMALL: the box
// spans less than 2^30 pixels, so every edge value fits in int32 (|e| <= 2 * span_x * span_y); otherwise int64.  The
// values are exact either way, so both forms give the same answer.
template <class T, T (*E)(int, int, int, int, int, int)>
__device__ __forceinline__ bool covers_t(const FaceRec& f, int px, int py) {
  const T e0 = E(f.x0, f.y0, f.x1, f.y1, px, py);
  const T e1 = E(f.x1, f.y1, f.x2, f.y2, px, py);
  const T e2 = E(f.x2, f.y2, f.x0, f.y0, px, py);
  if (!(f.flags & F_DEGENERATE)) return (e0 >= 0 && e1 >= 0 && e2 >= 0) || (e0 <= 0 && e1 <= 0 && e2 <= 0);
  // area 0: the integer points on the three segments
  const bool s0 = e0 == 0 && px >= min(f.x0, f.x1) && px <= max(f.x0, f.x1) && py >= min(f.y0, f.y1) && py <= max(f.y0, f.y1);
  const bool s1 = e1 == 0 && px >= min(f.x1, f.x2) && px <= max(f.x1, f.x2) && py >= min(f.y1, f.y2) && py <= max(f.y1, f.y2);
  const bool s2 = e2 == 0 && px >= min(f.x2, f.x0) && px <= max(f.x2, f.x0) && py >= min(f.y2, f.y0) && py <= max(f.y2, f.y0);
  return s0 || s1 || s2;
}
__device__ __forceinline__ bool covers(const FaceRec& f, int px, int py) {
  return (f.flags & F_SMALL) ? covers_t<int, edge32>(f, px, py) : covers_t<long long, edge64>(f, px, py);
}

// One workgroup per mesh of the block.
__global__ __launch_bounds__(256) void overlay_setup_kernel(MeshBlock mb, const double* __restrict__ K,
                                                            const double* __restrict__ verts, const int* __restrict__ faces,
                                                            int H, int W, int style, char* __restrict__ ws, Layout L) {
#pragma clang fp contract(off)
  const int mi = blockIdx.x, tid = threadIdx.x;
  const hm_mesh m = mb.m[mi];
  const double* k = K + (size_t)m.frame * 9;
  const double k00 = k[0], k01 = k[1], k02 = k[2], k10 = k[3], k11 = k[4], k12 = k[5], k20 = k[6], k21 = k[7], k22 = k[8];
  const double* vb = verts + (size_t)m.v0 * 3;
  FaceRec* recs = (FaceRec*)(ws + L.recs);
  int4* boxes = (int4*)(ws + L.boxes);
  unsigned* colours = (unsigned*)(ws + L.tail);
  int lx0 = INT_MAX, ly0 = INT_MAX, lx1 = INT_MIN, ly1 = INT_MIN;
  for (int j = tid; j < m.nf; j += 256) {
    const size_t fid = (size_t)m.f0 + j;
    const int c[3] = {faces[fid * 3], faces[fid * 3 + 1], faces[fid * 3 + 2]};
    bool ok = true;
    int px[3] = {0, 0, 0}, py[3] = {0, 0, 0};
    double X[3] = {0, 0, 0}, Y[3] = {0, 0, 0}, Z[3] = {0, 0, 0};
    for (int q = 0; q < 3; ++q) {
      if (c[q] < 0 || c[q] >= m.nv) { ok = false; continue; }       // never read outside the mesh's vertices
      const double x = vb[(size_t)c[q] * 3], y = vb[(size_t)c[q] * 3 + 1], z0 = vb[(size_t)c[q] * 3 + 2];
      const double z = z0 == 0.0 ? 1e-5 : z0;
      const double w = k20 * x + k21 * y + k22 * z;
      const double u = (k00 * x + k01 * y + k02 * z) / w;
      const double v = (k10 * x + k11 * y + k12 * z) / w;
      if (!(z0 > 0.0) || !(fabs(u) < 16777216.0) || !(fabs(v) < 16777216.0)) ok = false;
      else { px[q] = (int)u; py[q] = (int)v; }                     // truncation toward zero (astype(np.int32))
      X[q] = x; Y[q] = y; Z[q] = z;
    }
    int4 box = make_int4(1, 1, 0, 0);                                // empty
    FaceRec r = {px[0], py[0], px[1], py[1], px[2], py[2], 0u, 0};
    unsigned col = 0;
    if (ok) {
      const int fx0 = min(px[0], min(px[1], px[2])), fx1 = max(px[0], max(px[1], px[2]));
      const int fy0 = min(py[0], min(py[1], py[2])), fy1 = max(py[0], max(py[1], py[2]));
      const long long area = (long long)(px[1] - px[0]) * (py[2] - py[0]) - (long long)(py[1] - py[0]) * (px[2] - px[0]);
      const long long span = (long long)(fx1 - fx0 + 1) * (fy1 - fy0 + 1);
      r.flags = (area == 0 ? F_DEGENERATE : 0) | (span < (1ll << 30) ? F_SMALL : 0);
      r.depth = __float_as_uint((float)(((Z[0] + Z[1]) + Z[2]) / 3.0));
      box = make_int4(max(fx0, 0), max(fy0, 0), min(fx1, W - 1), min(fy1, H - 1));
      if (box.x <= box.z && box.y <= box.w) {
        lx0 = min(lx0, box.x); ly0 = min(ly0, box.y); lx1 = max(lx1, box.z); ly1 = max(ly1, box.w);
      }
      if (style == HM_STYLE_SHADED) {
        const double ax = X[1] - X[0], ay = Y[1] - Y[0], az = Z[1] - Z[0];
        const double cx = X[2] - X[0], cy = Y[2] - Y[0], cz = Z[2] - Z[0];
        const double nx = ay * cz - az * cy, ny = az * cx - ax * cz, nz = ax * cy - ay * cx;
        const double len = sqrt((nx * nx + ny * ny) + nz * nz);
        const double nzabs = len > 0.0 ? fabs(nz) / len : 0.0;
        const double I = 0.3 + 0.7 * nzabs;
        const unsigned b = rint_u8(255.0 * 0.9 * I), g = rint_u8(255.0 * 1.0 * I), rr = rint_u8(255.0 * 1.0 * I);
        col = b | (g << 8) | (rr << 16);
      } else {
        col = m.color_bgr[0] | ((unsigned)m.color_bgr[1] << 8) | ((unsigned)m.color_bgr[2] << 16);
      }
    }
    recs[fid] = r;
    boxes[fid] = box;
    colours[fid] = col;
  }
  emit_mesh_tiles(lx0, ly0, lx1, ly1, mb.first + mi, MeshRec{m.frame, m.f0, m.nf, 0}, ws, L);
}

// Grid-strided over the work list; one lane per pixel of a 16 x 16 tile.
__global__ __launch_bounds__(256) void overlay_raster_kernel(int H, int W, char* __restrict__ ws, Layout L) {
  __shared__ FaceRec s_face[256];
  const int tid = threadIdx.x;
  const unsigned count = *(const unsigned*)(ws + L.counter);
  const int2* items = (const int2*)(ws + L.items);
  const MeshRec* meshes = (const MeshRec*)(ws + L.meshes);
  const FaceRec* recs = (const FaceRec*)(ws + L.recs);
  const int4* boxes = (const int4*)(ws + L.boxes);
  for (unsigned w = blockIdx.x; w < count; w += gridDim.x) {
    const int2 it = items[w];
    const MeshRec m = meshes[it.x];
    const int tx = tile_x(it.y), ty = tile_y(it.y);
    const int x0 = tx * TILE, y0 = ty * TILE;
    const int px = x0 + (tid & (TILE - 1)), py = y0 + (tid >> 4);
    unsigned long long best = NO_KEY;
    for (int c0 = 0; c0 < m.nf; c0 += 256) {
      // cull 256 faces against the tile into the LDS list
      const int j = c0 + tid;
      const bool hit = j < m.nf && box_meets_tile(boxes[(size_t)m.f0 + j], x0, y0);
      const int n = cull_to_lds(hit, [&](int slot) {
        FaceRec r = recs[(size_t)m.f0 + j];
        r.flags |= j << 2;                                           // the face's index inside the mesh rides along
        s_face[slot] = r;
      });
      if (px < W && py < H) {
        for (int q = 0; q < n; ++q) {
          const FaceRec f = s_face[q];
          const int fx0 = min(f.x0, min(f.x1, f.x2)), fx1 = max(f.x0, max(f.x1, f.x2));
          const int fy0 = min(f.y0, min(f.y1, f.y2)), fy1 = max(f.y0, max(f.y1, f.y2));
          if (px < fx0 || px > fx1 || py < fy0 || py > fy1) continue;
          const unsigned long long key = ((unsigned long long)f.depth << 32) | (unsigned)(m.f0 + (f.flags >> 2));
          if (key < best && covers(f, px, py)) best = key;
        }
      }
      __syncthreads();                                               // the list is rewritten by the next chunk
    }
    if (best != NO_KEY) commit_key(ws, L, ((size_t)m.view * H + py) * W + px, tile_index(m.view, tx, ty, H, W), best);
  }
}

// Block (64, 4): 64 consecutive pixels of 4 rows; grid (ceil(W/64), ceil(H/4), N).
__global__ __launch_bounds__(256) void overlay_compose_kernel(const uint8_t* __restrict__ frames, uint8_t* __restrict__ out,
                                                              int H, int W, int style, float alpha, float beta,
                                                              char* __restrict__ ws, Layout L) {
#pragma clang fp contract(off)
  const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y, n = blockIdx.z;
  if (x >= W || y >= H) return;
  const size_t p = ((size_t)n * H + y) * W + x;
  const uint8_t* src = frames + p * 3;
  uint8_t* dst = out + p * 3;
  const uint8_t b = src[0], g = src[1], r = src[2];
  const unsigned long long key = take_key(ws, L, p, tile_index(n, x / TILE, y / TILE, H, W));
  if (key == NO_KEY) { dst[0] = b; dst[1] = g; dst[2] = r; return; }
  const unsigned col = ((const unsigned*)(ws + L.tail))[(unsigned)key];
  const unsigned cb = col & 255, cg = (col >> 8) & 255, cr = (col >> 16) & 255;
  if (style == HM_STYLE_SHADED) { dst[0] = cb; dst[1] = cg; dst[2] = cr; return; }
  // cv2.addWeighted(overlay, alpha, image, beta, 0): rint(alpha * c + beta * i) in fp32, product then sum
  const float ob = rintf(alpha * (float)cb + beta * (float)b);
  const float og = rintf(alpha * (float)cg + beta * (float)g);
  const float orr = rintf(alpha * (float)cr + beta * (float)r);
  dst[0] = (uint8_t)fminf(fmaxf(ob, 0.0f), 255.0f);
  dst[1] = (uint8_t)fminf(fmaxf(og, 0.0f), 255.0f);
  dst[2] = (uint8_t)fminf(fmaxf(orr, 0.0f), 255.0f);
}

int check_args(const uint8_t* frames, int N, int H, int W, const double* K, const double* verts, int n_verts, const int32_t* faces,
               int n_faces, const hm_mesh* meshes, int n_meshes, int style, double alpha, const uint8_t* out, const void* ws,
               size_t ws_bytes) {
  if (!frames || !K || !out || !ws) return hm_set_error(HM_ERR_ARG, "hm_mesh_overlay: null pointer");
  if (N <= 0 || N > 65535 || H <= 0 || W <= 0 || H > 32767 || W > 32767)
    return hm_set_error(HM_ERR_ARG, "hm_mesh_overlay: need 1 <= N <= 65535 and 1 <= H, W <= 32767");
  if (n_meshes < 0 || n_verts < 0 || n_faces < 0) return hm_set_error(HM_ERR_ARG, "hm_mesh_overlay: negative count");
  if (n_meshes > 0 && !meshes) return hm_set_error(HM_ERR_ARG, "hm_mesh_overlay: null mesh table");
  if ((n_verts > 0 && !verts) || (n_faces > 0 && !faces)) return hm_set_error(HM_ERR_ARG, "hm_mesh_overlay: null vertices or faces");
  if (style != HM_STYLE_FLAT && style != HM_STYLE_SHADED) return hm_set_error(HM_ERR_ARG, "hm_mesh_overlay: unknown style");
  if (!(alpha >= 0.0 && alpha <= 1.0)) return hm_set_error(HM_ERR_ARG, "hm_mesh_overlay: alpha outside [0, 1]");
  int rc = check_out_apart("hm_mesh_overlay", frames, out, (size_t)N * H * W * 3);
  if (rc == HM_OK) rc = check_mesh_table("hm_mesh_overlay", "frame", meshes, n_meshes, N, n_verts, n_faces, false);
  if (rc != HM_OK) return rc;
  if (ws_bytes < layout(N, H, W, n_meshes, n_faces).total) return hm_set_error(HM_ERR_ARG, "hm_mesh_overlay: workspace too small");
  return HM_OK;
}

}  // namespace

extern "C" size_t hm_mesh_overlay_workspace_bytes(int N, int H, int W, int n_meshes, int n_faces) {
  if (N <= 0 || H <= 0 || W <= 0 || n_meshes < 0 || n_faces < 0) return 0;
  return layout(N, H, W, n_meshes, n_faces).total;
}

extern "C" int hm_mesh_overlay(const uint8_t* frames, int N, int H, int W, const double* K, const double* verts, int n_verts,
                               const int32_t* faces, int n_faces, const hm_mesh* meshes_host, int n_meshes, int style,
                               double alpha, uint8_t* out, void* workspace, size_t workspace_bytes, void* stream_) {
  const int rc = check_args(frames, N, H, W, K, verts, n_verts, faces, n_faces, meshes_host, n_meshes, style, alpha, out, workspace,
                            workspace_bytes);
  if (rc != HM_OK) return rc;
  hipStream_t s = (hipStream_t)stream_;
  const Layout L = layout(N, H, W, n_meshes, n_faces);
  char* ws = (char*)workspace;
  HmProfScope prof(HM_K_OTHER, 0, N, H, W, s);
  if (hipMemsetAsync(ws + L.counter, 0, L.meshes - L.counter, s) != hipSuccess)     // counter and tile flags
    return hm_set_error(HM_ERR_HIP, "hm_mesh_overlay: hipMemsetAsync");
  for (int first = 0; first < n_meshes; first += MESHES_PER_LAUNCH) {
    MeshBlock mb;
    mb.first = first;
    mb.count = n_meshes - first < MESHES_PER_LAUNCH ? n_meshes - first : MESHES_PER_LAUNCH;
    for (int i = 0; i < mb.count; ++i) mb.m[i] = meshes_host[first + i];
    hipLaunchKernelGGL(overlay_setup_kernel, dim3(mb.count), dim3(256), 0, s, mb, K, verts, faces, H, W, style, ws, L);
  }
  if (n_meshes > 0) hipLaunchKernelGGL(overlay_raster_kernel, dim3(raster_grid(n_meshes, H, W)), dim3(256), 0, s, H, W, ws, L);
  const float a = (float)alpha, b = (float)(1.0 - alpha);
  hipLaunchKernelGGL(overlay_compose_kernel, dim3((W + 63) / 64, (H + 3) / 4, N), dim3(64, 4), 0, s, frames, out, H, W, style, a, b,
                     ws, L);
  return hm_check_launch("hm_mesh_overlay");
}
