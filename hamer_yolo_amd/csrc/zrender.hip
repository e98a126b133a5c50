// Z-buffered mesh renderer (reference: hamer/utils/mesh_renderer.py MeshRenderer.__call__, :243-320, `color, rend_depth =
// renderer.render(...)`): per view an RGBA image, a per-pixel depth map and a per-pixel mesh label, and optionally the
// colour composed onto BGR frames.  The rule is stated in include/hamer_hip.h (hm_mesh_render) and DESIGN.md section 8.1;
// tests/zrender_rule.py restates it in numpy.  It has the shape of render.hip, and the common part is raster_tiles.h: one
// workspace whose key buffer stays 0xFF between calls, mesh records as kernel arguments, no host synchronisation.  Which
// pixel centres a face covers is zbuffer_faces.h, shared with visibility.hip.
//  * normals - one thread per vertex walks its mesh's faces, staged in LDS 1024 at a time, and sums the fp64 face cross
//              products of the faces that name it in ascending row order: no float atomics, one order.
//  * setup   - one workgroup per mesh: the shared face setup, of which this file keeps everything (1/z per corner, the area,
//              the vertex rows); the mesh's box, cut into 16 x 16 tiles, appended to a work list through one atomic counter.
//  * raster  - a grid-strided loop over the work list: per (mesh, tile) the faces are culled into LDS (ballot + prefix),
//              one lane per pixel runs the shared sample test, computes the fp64 perspective-correct depth of the covered
//              (pixel, face) pairs only, and sends the smallest (fp32 depth bits, face id) key to the view's key buffer with
//              one unsigned 64-bit atomicMin.
//  * resolve - one pass over the views, four pixels per lane where the row length and the pointers allow 16-byte
//              accesses: keys are read and reset in flagged tiles only, the winning face's barycentrics are recomputed, the
//              vertex normals interpolated and shaded, and the requested outputs written.
// The whole file is compiled without contraction, and every fp64 expression is written in the rule's order.
#include <math.h>
#include "common.h"
#include "raster_tiles.h"
#include "zbuffer_faces.h"

#pragma clang fp contract(off)

namespace {
using namespace raster_tiles;
using namespace zbuffer_faces;

constexpr int NORMAL_CHUNK = 1024;                 // faces staged in LDS per step of the normals kernel

// Per face, written by setup, indexed by the global face id.
struct ZFace {
  FaceGeom g;                                      // g.tag: row of the mesh table
  double area2;                                    // twice the area (> 0), exact
  double r0, r1, r2;                               // 1 / z per corner
  int v0, v1, v2, pad;                             // global vertex rows of the corners
};
struct ZTileFace {                                 // what raster keeps in LDS
  FaceGeom g;                                      // g.tag: the face's index inside its mesh
  double area2, r0, r1, r2;
};
static_assert(sizeof(ZFace) == 80 && sizeof(ZTileFace) == 64, "the workspace layout counts on these");

using ZLayout = TileLayout;                        // tail: one fp64 normal (three doubles) per vertex
ZLayout layout(int N, int H, int W, int n_verts, int n_meshes, int n_faces) {
  return tile_layout(N, H, W, n_meshes, n_faces, sizeof(ZFace), (size_t)n_verts * 3 * sizeof(double));
}

// Grid (ceil(max nv / 256), meshes of the block): one thread per vertex.
__global__ __launch_bounds__(256) void zrender_normals_kernel(MeshBlock mb, const double* __restrict__ verts, const int* __restrict__ faces,
                                                              char* __restrict__ ws, ZLayout L) {
  __shared__ int s_f[NORMAL_CHUNK * 3];
  const hm_mesh m = mb.m[blockIdx.y].m;
  if ((int)(blockIdx.x * 256) >= m.nv) return;                         // the whole workgroup leaves together
  const int tid = threadIdx.x, v = blockIdx.x * 256 + tid;
  const double* vb = verts + (size_t)m.v0 * 3;
  double nx = 0.0, ny = 0.0, nz = 0.0;
  for (int c0 = 0; c0 < m.nf; c0 += NORMAL_CHUNK) {
    const int n = min(NORMAL_CHUNK, m.nf - c0);
    for (int j = tid; j < n; j += 256) {
      const size_t fid = (size_t)m.f0 + c0 + j;
      const int a = faces[fid * 3], b = faces[fid * 3 + 1], c = faces[fid * 3 + 2];
      const bool ok = a >= 0 && a < m.nv && b >= 0 && b < m.nv && c >= 0 && c < m.nv;
      s_f[j * 3] = ok ? a : -1; s_f[j * 3 + 1] = ok ? b : -1; s_f[j * 3 + 2] = ok ? c : -1;
    }
    __syncthreads();
    if (v < m.nv) {
      for (int j = 0; j < n; ++j) {
        const int a = s_f[j * 3], b = s_f[j * 3 + 1], c = s_f[j * 3 + 2];
        if (a != v && b != v && c != v) continue;
        const double* p0 = vb + (size_t)a * 3;
        const double* p1 = vb + (size_t)b * 3;
        const double* p2 = vb + (size_t)c * 3;
        const double ax = p1[0] - p0[0], ay = p1[1] - p0[1], az = p1[2] - p0[2];
        const double cx = p2[0] - p0[0], cy = p2[1] - p0[1], cz = p2[2] - p0[2];
        nx = nx + (ay * cz - az * cy);
        ny = ny + (az * cx - ax * cz);
        nz = nz + (ax * cy - ay * cx);
      }
    }
    __syncthreads();                                                   // the list is rewritten by the next chunk
  }
  if (v < m.nv) {
    double* out = (double*)(ws + L.tail) + ((size_t)m.v0 + v) * 3;
    out[0] = nx; out[1] = ny; out[2] = nz;
  }
}

// One workgroup per mesh of the block.
__global__ __launch_bounds__(256) void zrender_setup_kernel(MeshBlock mb, const double* __restrict__ verts,
                                                            const int* __restrict__ faces, int H, int W, double znear,
                                                            char* __restrict__ ws, ZLayout L) {
  const int mi = blockIdx.x, mesh = mb.first + mi;
  const hm_mesh m = mb.m[mi].m;
  const int4 box = setup_faces(mb.m[mi], verts, faces, H, W, znear, (ZFace*)(ws + L.recs), (int4*)(ws + L.boxes),
                               [&](ZFace& r, const FaceGeom& g, const FaceRest& t) {
    r.g = g; r.g.tag = mesh; r.area2 = t.area2;
    r.r0 = t.r0; r.r1 = t.r1; r.r2 = t.r2;
    r.v0 = m.v0 + t.c0; r.v1 = m.v0 + t.c1; r.v2 = m.v0 + t.c2;
  });
  emit_mesh_tiles(box.x, box.y, box.z, box.w, mesh, MeshRec{m.frame, m.f0, m.nf, 0}, ws, L);
}

// fp32 depth of a covered sample from its edge values: the rule's expression, in its order.
__device__ __forceinline__ float sample_depth(double e0, double e1, double e2, double area2, double r0, double r1, double r2) {
  const double l0 = e0 / area2, l1 = e1 / area2, l2 = e2 / area2;
  const double q = (l0 * r0 + l1 * r1) + l2 * r2;
  return (float)(1.0 / q);
}

// Grid-strided over the work list; one lane per pixel of a 16 x 16 tile.
__global__ __launch_bounds__(256) void zrender_raster_kernel(int H, int W, char* __restrict__ ws, ZLayout L) {
  __shared__ ZTileFace s_face[256];
  const int tid = threadIdx.x;
  const unsigned count = *(const unsigned*)(ws + L.counter);
  const int2* items = (const int2*)(ws + L.items);
  const MeshRec* meshes = (const MeshRec*)(ws + L.meshes);
  const ZFace* recs = (const ZFace*)(ws + L.recs);
  const int4* boxes = (const int4*)(ws + L.boxes);
  for (unsigned w = blockIdx.x; w < count; w += gridDim.x) {
    const int2 it = items[w];
    const MeshRec m = meshes[it.x];
    const int tx = tile_x(it.y), ty = tile_y(it.y);
    const int x0 = tx * TILE, y0 = ty * TILE;
    const int px = x0 + (tid & (TILE - 1)), py = y0 + (tid >> 4);
    const int sx = 256 * px + 128, sy = 256 * py + 128;                // the sample: the pixel's centre
    unsigned long long best = NO_KEY;
    for (int c0 = 0; c0 < m.nf; c0 += 256) {
      // cull 256 faces against the tile into the LDS list
      const int j = c0 + tid;
      const bool hit = j < m.nf && box_meets_tile(boxes[(size_t)m.f0 + j], x0, y0);
      const int n = cull_to_lds(hit, [&](int slot) {
        const ZFace r = recs[(size_t)m.f0 + j];
        const FaceGeom& g = r.g;                                       // member by member: the record leaves as four 16-byte stores
        const ZTileFace t = {{g.x0, g.y0, g.x1, g.y1, g.x2, g.y2, g.flags, j}, r.area2, r.r0, r.r1, r.r2};
        s_face[slot] = t;
      });
      if (px < W && py < H) {
        for (int q = 0; q < n; ++q) {
          const ZTileFace& f = s_face[q];
          double e0, e1, e2;
          if (outside_box(f.g, sx, sy)) continue;
          if (!edges_inside(f.g, sx, sy, e0, e1, e2)) continue;
          const float d = sample_depth(e0, e1, e2, f.area2, f.r0, f.r1, f.r2);
          const unsigned long long key = ((unsigned long long)__float_as_uint(d) << 32) | (unsigned)(m.f0 + f.g.tag);
          if (key < best) best = key;
        }
      }
      __syncthreads();                                               // the list is rewritten by the next chunk
    }
    if (best != NO_KEY) commit_key(ws, L, ((size_t)m.view * H + py) * W + px, tile_index(m.view, tx, ty, H, W), best);
  }
}

struct ZOut {
  const uint8_t* frames;
  uint8_t* out;
  uint8_t* rgba;
  float* depth;
  int* mesh_id;
  double base[3];
  unsigned bg;                                     // R | G << 8 | B << 16 | A << 24: the bytes of an uncovered RGBA pixel
};

struct ZPixel { unsigned rgba; float depth; int mesh; };

// The winning face of pixel (px, py), shaded.
__device__ __forceinline__ ZPixel shade(unsigned long long key, int px, int py, const ZOut& o, const char* __restrict__ ws,
                                        const ZLayout& L) {
  const ZFace f = ((const ZFace*)(ws + L.recs))[(unsigned)key];
  const double* nrm = (const double*)(ws + L.tail);
  const int sx = 256 * px + 128, sy = 256 * py + 128;
  const FaceGeom& g = f.g;
  const double e0 = (double)edge64(g.x1, g.y1, g.x2, g.y2, sx, sy), e1 = (double)edge64(g.x2, g.y2, g.x0, g.y0, sx, sy),
               e2 = (double)edge64(g.x0, g.y0, g.x1, g.y1, sx, sy);
  const double l0 = e0 / f.area2, l1 = e1 / f.area2, l2 = e2 / f.area2;
  const double a0 = l0 * f.r0, a1 = l1 * f.r1, a2 = l2 * f.r2;
  const double* n0 = nrm + (size_t)f.v0 * 3;
  const double* n1 = nrm + (size_t)f.v1 * 3;
  const double* n2 = nrm + (size_t)f.v2 * 3;
  const double mx = (a0 * n0[0] + a1 * n1[0]) + a2 * n2[0];
  const double my = (a0 * n0[1] + a1 * n1[1]) + a2 * n2[1];
  const double mz = (a0 * n0[2] + a1 * n1[2]) + a2 * n2[2];
  const double len = sqrt((mx * mx + my * my) + mz * mz);
  const double t = len > 0.0 ? fabs(mz) / len : 0.0;
  const double I = 0.3 + 0.7 * t;
  ZPixel p;
  p.rgba = rint_u8(255.0 * o.base[0] * I) | (rint_u8(255.0 * o.base[1] * I) << 8) | (rint_u8(255.0 * o.base[2] * I) << 16) | 0xFF000000u;
  p.depth = __uint_as_float((unsigned)(key >> 32));
  p.mesh = f.g.tag;
  return p;
}

// Block (64, 4); a lane owns PX consecutive pixels of one row (PX = 4: W % 4 == 0 and every pointer 16-byte aligned, so the
// keys, RGBA, depth and label rows move 16 bytes at a time and the BGR rows 12).  Grid (ceil(W / (64 PX)), ceil(H / 4), N).
template <int PX>
__global__ __launch_bounds__(256) void zrender_resolve_kernel(ZOut o, int H, int W, char* __restrict__ ws, ZLayout L) {
  const int x = (blockIdx.x * 64 + threadIdx.x) * PX, y = blockIdx.y * 4 + threadIdx.y, n = blockIdx.z;
  if (x >= W || y >= H) return;
  const size_t p = ((size_t)n * H + y) * W + x;
  const size_t tile = tile_index(n, x / TILE, y / TILE, H, W);         // PX divides TILE: a lane's pixels share a tile
  unsigned long long key[PX];
  if (PX == 1) {
    key[0] = take_key(ws, L, p, tile);
  } else {
    // take_key's rule (raster_tiles.h), 16 bytes at a time: flagged tiles only, and the four keys are reset if one was set
#pragma unroll
    for (int i = 0; i < PX; ++i) key[i] = NO_KEY;
    if (((const unsigned char*)(ws + L.flags))[tile]) {
      unsigned long long* kp = (unsigned long long*)(ws + L.keys) + p;
      const ulonglong2 a = ((const ulonglong2*)kp)[0], b = ((const ulonglong2*)kp)[1];
      key[0] = a.x; key[1 % PX] = a.y; key[2 % PX] = b.x; key[3 % PX] = b.y;
      if ((a.x & a.y & b.x & b.y) != NO_KEY) {
        const ulonglong2 ff = make_ulonglong2(NO_KEY, NO_KEY);
        ((ulonglong2*)kp)[0] = ff; ((ulonglong2*)kp)[1] = ff;
      }
    }
  }
  unsigned rgba[PX];
  float depth[PX];
  int mesh[PX];
  bool hit[PX];
#pragma unroll
  for (int i = 0; i < PX; ++i) {
    hit[i] = key[i] != NO_KEY;
    rgba[i] = o.bg; depth[i] = 0.0f; mesh[i] = -1;
    if (hit[i]) {
      const ZPixel s = shade(key[i], x + i, y, o, ws, L);
      rgba[i] = s.rgba; depth[i] = s.depth; mesh[i] = s.mesh;
    }
  }
  if (PX == 4) {
    if (o.rgba) *(uint4*)(o.rgba + p * 4) = make_uint4(rgba[0], rgba[1 % PX], rgba[2 % PX], rgba[3 % PX]);
    if (o.depth) *(float4*)(o.depth + p) = make_float4(depth[0], depth[1 % PX], depth[2 % PX], depth[3 % PX]);
    if (o.mesh_id) *(int4*)(o.mesh_id + p) = make_int4(mesh[0], mesh[1 % PX], mesh[2 % PX], mesh[3 % PX]);
    if (o.out) {
      const unsigned* src = (const unsigned*)(o.frames + p * 3);       // 12 bytes: B G R B | G R B G | R B G R
      const unsigned wds[3] = {src[0], src[1], src[2]};
      unsigned b[12];                                                  // unrolled: the bytes stay in registers
#pragma unroll
      for (int k = 0; k < 12; ++k) b[k] = (wds[k >> 2] >> (8 * (k & 3))) & 255u;
#pragma unroll
      for (int i = 0; i < PX; ++i)
        if (hit[i]) { b[i * 3] = (rgba[i] >> 16) & 255u; b[i * 3 + 1] = (rgba[i] >> 8) & 255u; b[i * 3 + 2] = rgba[i] & 255u; }
      unsigned* dst = (unsigned*)(o.out + p * 3);
#pragma unroll
      for (int k = 0; k < 3; ++k) dst[k] = b[4 * k] | (b[4 * k + 1] << 8) | (b[4 * k + 2] << 16) | (b[4 * k + 3] << 24);
    }
  } else {
    if (o.rgba) *(unsigned*)(o.rgba + p * 4) = rgba[0];
    if (o.depth) o.depth[p] = depth[0];
    if (o.mesh_id) o.mesh_id[p] = mesh[0];
    if (o.out) {
      const uint8_t* src = o.frames + p * 3;
      uint8_t* dst = o.out + p * 3;
      dst[0] = hit[0] ? (uint8_t)(rgba[0] >> 16) : src[0];
      dst[1] = hit[0] ? (uint8_t)(rgba[0] >> 8) : src[1];
      dst[2] = hit[0] ? (uint8_t)rgba[0] : src[2];
    }
  }
}

int check_args(int N, int H, int W, const double* K, const double* verts, int n_verts, const int32_t* faces, int n_faces,
               const hm_mesh* meshes, int n_meshes, const double* base_rgb, double znear, const uint8_t* frames, const uint8_t* out,
               const uint8_t* rgba, const float* depth, const int32_t* mesh_id, const void* ws, size_t ws_bytes) {
  if (!K || !ws) return hm_set_error(HM_ERR_ARG, "hm_mesh_render: null pointer");
  // the keys take 64-bit atomics and the face records hold doubles; the one-pixel resolve stores whole words
  if ((uintptr_t)ws & 7) return hm_set_error(HM_ERR_ARG, "hm_mesh_render: workspace must be 8-byte aligned");
  if (((uintptr_t)rgba | (uintptr_t)depth | (uintptr_t)mesh_id) & 3)
    return hm_set_error(HM_ERR_ARG, "hm_mesh_render: rgba, depth and mesh_id must be 4-byte aligned");
  if (((uintptr_t)verts & 7) || ((uintptr_t)faces & 3)) return hm_set_error(HM_ERR_ARG, "hm_mesh_render: verts must be 8-byte, faces 4-byte aligned");
  if (N <= 0 || N > 65535 || H <= 0 || W <= 0 || H > 32767 || W > 32767)
    return hm_set_error(HM_ERR_ARG, "hm_mesh_render: need 1 <= N <= 65535 and 1 <= H, W <= 32767");
  if (n_meshes < 0 || n_verts < 0 || n_faces < 0) return hm_set_error(HM_ERR_ARG, "hm_mesh_render: negative count");
  if (n_meshes > 0 && !meshes) return hm_set_error(HM_ERR_ARG, "hm_mesh_render: null mesh table");
  if ((n_verts > 0 && !verts) || (n_faces > 0 && !faces)) return hm_set_error(HM_ERR_ARG, "hm_mesh_render: null vertices or faces");
  if (!positive_finite(znear)) return hm_set_error(HM_ERR_ARG, "hm_mesh_render: znear must be a finite number > 0");
  int rc = check_cameras("hm_mesh_render", K, N);
  if (rc != HM_OK) return rc;
  if (base_rgb)
    for (int c = 0; c < 3; ++c)
      if (!(base_rgb[c] >= 0.0 && base_rgb[c] <= 1.0)) return hm_set_error(HM_ERR_ARG, "hm_mesh_render: base_rgb outside [0, 1]");
  if (!out && !rgba && !depth && !mesh_id) return hm_set_error(HM_ERR_ARG, "hm_mesh_render: no output requested");
  if ((frames == nullptr) != (out == nullptr)) return hm_set_error(HM_ERR_ARG, "hm_mesh_render: frames and out are given both or neither");
  rc = check_out_apart("hm_mesh_render", frames, out, (size_t)N * H * W * 3);
  if (rc == HM_OK) rc = check_mesh_table("hm_mesh_render", "view", meshes, n_meshes, N, n_verts, n_faces, true);
  if (rc != HM_OK) return rc;
  if (ws_bytes < layout(N, H, W, n_verts, n_meshes, n_faces).total) return hm_set_error(HM_ERR_ARG, "hm_mesh_render: workspace too small");
  return HM_OK;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" size_t hm_mesh_render_workspace_bytes(int N, int H, int W, int n_verts, int n_meshes, int n_faces) {
  if (N <= 0 || H <= 0 || W <= 0 || n_verts < 0 || n_meshes < 0 || n_faces < 0) return 0;
  return layout(N, H, W, n_verts, n_meshes, n_faces).total;
}

extern "C" int hm_mesh_render(int N, int H, int W, const double* K_host, const double* verts, int n_verts, const int32_t* faces,
                              int n_faces, const hm_mesh* meshes_host, int n_meshes, const double* base_rgb, const uint8_t* bg_rgba,
                              double znear, const uint8_t* frames, uint8_t* out, uint8_t* rgba, float* depth, int32_t* mesh_id,
                              void* workspace, size_t workspace_bytes, void* stream_) {
  const int rc = check_args(N, H, W, K_host, verts, n_verts, faces, n_faces, meshes_host, n_meshes, base_rgb, znear, frames, out, rgba,
                            depth, mesh_id, workspace, workspace_bytes);
  if (rc != HM_OK) return rc;
  hipStream_t s = (hipStream_t)stream_;
  const ZLayout L = layout(N, H, W, n_verts, n_meshes, n_faces);
  char* ws = (char*)workspace;
  HmProfScope prof(HM_K_OTHER, 1, N, H, W, s);
  if (hipMemsetAsync(ws + L.counter, 0, L.meshes - L.counter, s) != hipSuccess)     // counter and tile flags
    return hm_set_error(HM_ERR_HIP, "hm_mesh_render: hipMemsetAsync");
  for (int first = 0; first < n_meshes; first += MESHES_PER_LAUNCH) {
    MeshBlock mb;
    const int max_nv = fill_mesh_block(mb, meshes_host, n_meshes, K_host, first);
    if (max_nv > 0)
      hipLaunchKernelGGL(zrender_normals_kernel, dim3((max_nv + 255) / 256, mb.count), dim3(256), 0, s, mb, verts, faces, ws, L);
    hipLaunchKernelGGL(zrender_setup_kernel, dim3(mb.count), dim3(256), 0, s, mb, verts, faces, H, W, znear, ws, L);
  }
  if (n_meshes > 0) hipLaunchKernelGGL(zrender_raster_kernel, dim3(raster_grid(n_meshes, H, W)), dim3(256), 0, s, H, W, ws, L);
  ZOut o;
  o.frames = frames; o.out = out; o.rgba = rgba; o.depth = depth; o.mesh_id = mesh_id;
  o.base[0] = base_rgb ? base_rgb[0] : 1.0; o.base[1] = base_rgb ? base_rgb[1] : 1.0; o.base[2] = base_rgb ? base_rgb[2] : 0.9;
  o.bg = bg_rgba ? (unsigned)bg_rgba[0] | ((unsigned)bg_rgba[1] << 8) | ((unsigned)bg_rgba[2] << 16) | ((unsigned)bg_rgba[3] << 24) : 0u;
  const bool vec = W % 4 == 0 && aligned16(ws) && aligned16(rgba) && aligned16(depth) && aligned16(mesh_id) &&
                   ((uintptr_t)frames & 3) == 0 && ((uintptr_t)out & 3) == 0;
  if (vec)
    hipLaunchKernelGGL(zrender_resolve_kernel<4>, dim3((W + 255) / 256, (H + 3) / 4, N), dim3(64, 4), 0, s, o, H, W, ws, L);
  else
    hipLaunchKernelGGL(zrender_resolve_kernel<1>, dim3((W + 63) / 64, (H + 3) / 4, N), dim3(64, 4), 0, s, o, H, W, ws, L);
  return hm_check_launch("hm_mesh_render");
}
