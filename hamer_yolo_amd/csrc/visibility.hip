// What the camera sees of each hand: a visibility code per 3-D point and pixel counts and boxes per
// mesh, both against the depth and label maps hm_mesh_render writes, and optionally a sensor depth map and a label mask.
// The rules are stated in include/hamer_hip.h ("Visibility"); tests/visibility_rule.py restates them in numpy.
//  * hm_point_visibility - an init kernel writes every group's count row (zeros and np); the point kernel runs one lane per
//                point over the (group, 256-point chunk) items, found by a scan of the group table: the renderer's projection
//                (zbuffer_faces.h), the window tests, one code byte per point; the counts are ballot popcounts added up in
//                LDS, then one integer atomic per occupied code and chunk.  The cameras travel as kernel arguments, 64 views
//                per launch.
//  * hm_mesh_coverage - the renderer's face setup and sample test (zbuffer_faces.h), of which only the geometry is kept, then
//                one pass over the work list: per (mesh, tile) the faces are culled into LDS, one lane per pixel decides "any
//                face of the mesh covers my centre", classifies the pixel against the maps, and the workgroup sends ballot
//                popcounts (64-bit adds) and the boxes' corners (32-bit min / max).  No key buffer, no per-pixel output.
// The whole file is compiled without contraction, and every fp64 expression is written in the rule's order.
#include <math.h>
#include "common.h"
#include "raster_tiles.h"
#include "zbuffer_faces.h"

#pragma clang fp contract(off)

namespace {
using namespace raster_tiles;
using namespace zbuffer_faces;

constexpr int VIEWS_PER_LAUNCH = 64;               // 64 cameras of six doubles: the argument block stays under 4 KiB
enum { VIS_VISIBLE = 0, VIS_BEHIND, VIS_OUTSIDE, VIS_SELF, VIS_OTHER, VIS_SCENE, VIS_OFF_MASK };

struct VisCameras {
  double k[VIEWS_PER_LAUNCH][6];                   // K00 K01 K02 K10 K11 K12 of views first .. first + count - 1
  int first, count;
};
struct VisMaps {
  const float* depth;
  const int32_t* mesh_id;
  const uint16_t* sensor;                          // or null
  const uint8_t* mask;                             // or null
  double unit, scene_tol_m;
  int raw_lo, raw_hi;
  int N, H, W;
};

// label -1: mask != 0; 0..255: mask == label; anything else: no pixel passes (-2 is handled by the caller)
__device__ __forceinline__ bool mask_passes(int value, int label) {
  return label == -1 ? value != 0 : (label >= 0 && label <= 255 && value == label);
}
__device__ __forceinline__ bool reading_valid(int raw, int raw_lo, int raw_hi) { return raw != 0 && raw >= raw_lo && raw <= raw_hi; }

// A group's points, as the kernels read them: a range that leaves [0, P) counts as empty, so nothing outside is touched.
__device__ __forceinline__ int group_points(const hm_vis_group& g, int P) {
  return (g.np > 0 && g.p0 >= 0 && (long long)g.p0 + g.np <= (long long)P) ? g.np : 0;
}

__global__ __launch_bounds__(256) void vis_counts_init_kernel(const hm_vis_group* __restrict__ groups, int G, int P,
                                                              int32_t* __restrict__ counts) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= G * 8) return;
  counts[i] = (i & 7) == 7 ? group_points(groups[i >> 3], P) : 0;
}

__device__ __forceinline__ int point_code(const hm_vis_group& g, const double* __restrict__ pt, const VisCameras& cam,
                                          const VisMaps& m, double znear, int window) {
  const double x = pt[0], y = pt[1], z = pt[2];
  if (!(z >= znear)) return VIS_BEHIND;
  if (g.view < 0 || g.view >= m.N) return VIS_OUTSIDE;
  int X, Y;
  if (!project_fixed(cam.k[g.view - cam.first], x, y, z, X, Y)) return VIS_OUTSIDE;
  const int px = X >> 8, py = Y >> 8;                                  // arithmetic shifts: floor
  if (px < 0 || px >= m.W || py < 0 || py >= m.H) return VIS_OUTSIDE;
  const size_t base = (size_t)g.view * m.H * m.W;
  const int x0 = max(px - window, 0), x1 = min(px + window, m.W - 1);
  const int y0 = max(py - window, 0), y1 = min(py + window, m.H - 1);
  const double zt = z - g.tol_m;
  bool pass = false;
  for (int yy = y0; yy <= y1; ++yy)
    for (int xx = x0; xx <= x1; ++xx) {
      const size_t p = base + (size_t)yy * m.W + xx;
      if (m.mesh_id[p] >= 0) pass = pass || (double)m.depth[p] >= zt;
      else pass = pass || (xx == px && yy == py);
    }
  const size_t centre = base + (size_t)py * m.W + px;
  if (!pass) return m.mesh_id[centre] == g.mesh ? VIS_SELF : VIS_OTHER;
  if (m.sensor) {
    const double zs = z - m.scene_tol_m;
    bool any = false, clear = false;
    for (int yy = y0; yy <= y1; ++yy)
      for (int xx = x0; xx <= x1; ++xx) {
        const int raw = m.sensor[base + (size_t)yy * m.W + xx];
        if (!reading_valid(raw, m.raw_lo, m.raw_hi)) continue;
        any = true;
        clear = clear || (double)raw * m.unit >= zs;
      }
    if (any && !clear) return VIS_SCENE;
  }
  if (m.mask && g.label != -2 && !mask_passes(m.mask[centre], g.label)) return VIS_OFF_MASK;
  return VIS_VISIBLE;
}

// Work items are (group, chunk of 256 points), numbered in table order; workgroup b takes the items b, b + grid, ...  Every
// workgroup walks the whole table (uniform loads) to find them.  A launch handles the groups whose view lies in its block of
// cameras; the first launch also takes the groups whose view lies outside the batch.
__global__ __launch_bounds__(256) void vis_points_kernel(VisCameras cam, VisMaps m, double znear, int window,
                                                         const double* __restrict__ points, int P,
                                                         const hm_vis_group* __restrict__ groups, int G,
                                                         uint8_t* __restrict__ codes, int32_t* __restrict__ counts) {
  __shared__ int s_cnt[8];
  const int tid = threadIdx.x, lane = tid & 63;
  const unsigned grid = gridDim.x, bid = blockIdx.x;
  unsigned item = 0;
  for (int gi = 0; gi < G; ++gi) {
    const hm_vis_group g = groups[gi];
    const int np = group_points(g, P);
    const unsigned nch = ((unsigned)np + 255u) / 256u;
    const unsigned first = (bid + grid - item % grid) % grid;           // this workgroup's first chunk of the group
    item += nch;
    const bool in_batch = g.view >= 0 && g.view < m.N;
    const bool mine = in_batch ? (g.view >= cam.first && g.view < cam.first + cam.count) : cam.first == 0;
    if (!mine) continue;
    for (unsigned c = first; c < nch; c += grid) {
      if (tid < 8) s_cnt[tid] = 0;
      __syncthreads();
      const int i = (int)(c * 256u) + tid;
      int code = -1;
      if (i < np) {
        code = point_code(g, points + ((size_t)g.p0 + i) * 3, cam, m, znear, window);
        codes[(size_t)g.p0 + i] = (uint8_t)code;
      }
      for (int k = 0; k < 7; ++k) {
        const unsigned long long b = __ballot(code == k);
        if (lane == 0 && b) atomicAdd(&s_cnt[k], __popcll(b));
      }
      __syncthreads();
      if (tid < 7 && s_cnt[tid]) atomicAdd(&counts[(size_t)gi * 8 + tid], s_cnt[tid]);
      __syncthreads();                                                  // s_cnt is cleared by the next chunk
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------ coverage
using CFace = FaceGeom;                            // a face record is the geometry alone (tag unused: 0)
static_assert(sizeof(CFace) == 32, "the workspace layout counts on this");

// The tile core's workspace without its key buffer and tile flags: counter, mesh records, work list, face records, face boxes.
TileLayout layout(int H, int W, int n_meshes, int n_faces) {
  const size_t tiles = tiles_of(H, W);
  TileLayout L;
  L.keys = 0; L.counter = 0; L.flags = 256;
  L.meshes = 256;
  L.items = align256(L.meshes + (size_t)n_meshes * sizeof(MeshRec));
  L.recs = align256(L.items + (size_t)n_meshes * tiles * sizeof(int2));
  L.boxes = align256(L.recs + (size_t)n_faces * sizeof(CFace));
  L.tail = align256(L.boxes + (size_t)n_faces * sizeof(int4));
  L.total = L.tail;
  return L;
}

// One workgroup per mesh of the block.
__global__ __launch_bounds__(256) void coverage_setup_kernel(MeshBlock mb, const double* __restrict__ verts,
                                                             const int* __restrict__ faces, int H, int W, double znear,
                                                             char* __restrict__ ws, TileLayout L) {
  const int mi = blockIdx.x;
  const hm_mesh m = mb.m[mi].m;
  const int4 box = setup_faces(mb.m[mi], verts, faces, H, W, znear, (CFace*)(ws + L.recs), (int4*)(ws + L.boxes),
                               [](CFace& r, const FaceGeom& g, const FaceRest&) { r = g; });
  emit_mesh_tiles(box.x, box.y, box.z, box.w, mb.first + mi, MeshRec{m.frame, m.f0, m.nf, 0}, ws, L);
}

// The box of a wave's set lanes inside its four tile rows (lane = 16 * row + column): left, top, right, bottom, tile-relative.
__device__ __forceinline__ int4 ballot_box(unsigned long long b, int wave) {
  const unsigned cols = (unsigned)((b | (b >> 16) | (b >> 32) | (b >> 48)) & 0xFFFFull);
  return make_int4(__ffs(cols) - 1, wave * 4 + ((__ffsll((unsigned long long)b) - 1) >> 4), 31 - __clz(cols),
                   wave * 4 + ((63 - __clzll((long long)b)) >> 4));
}

struct CoverageOut {
  unsigned long long* counts;                      // [n_meshes][8], zero on entry
  unsigned* boxes;                                 // [n_meshes][8], 0xFFFFFFFF (= -1) on entry
  const int32_t* labels;                           // or null
};

// Grid-strided over the work list; one lane per pixel of a 16 x 16 tile.
__global__ __launch_bounds__(256) void coverage_kernel(VisMaps mp, CoverageOut o, char* __restrict__ ws, TileLayout L) {
  __shared__ CFace s_face[256];
  __shared__ int s_cnt[8];
  __shared__ int s_box[8];                                               // amodal x1 y1 x2 y2, modal x1 y1 x2 y2
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int H = mp.H, W = mp.W;
  const unsigned count = *(const unsigned*)(ws + L.counter);
  const int2* items = (const int2*)(ws + L.items);
  const MeshRec* meshes = (const MeshRec*)(ws + L.meshes);
  const CFace* recs = (const CFace*)(ws + L.recs);
  const int4* boxes = (const int4*)(ws + L.boxes);
  for (unsigned w = blockIdx.x; w < count; w += gridDim.x) {
    const int2 it = items[w];
    const MeshRec m = meshes[it.x];
    const int x0 = tile_x(it.y) * TILE, y0 = tile_y(it.y) * TILE;
    const int px = x0 + (tid & (TILE - 1)), py = y0 + (tid >> 4);
    const int sx = 256 * px + 128, sy = 256 * py + 128;                // the sample: the pixel's centre
    const bool in_view = px < W && py < H;
    if (tid < 8) { s_cnt[tid] = 0; s_box[tid] = (tid & 2) ? -1 : INT_MAX; }
    bool cov = false;
    for (int c0 = 0; c0 < m.nf; c0 += 256) {
      const int j = c0 + tid;
      const bool hit = j < m.nf && box_meets_tile(boxes[(size_t)m.f0 + j], x0, y0);
      const int n = cull_to_lds(hit, [&](int slot) { s_face[slot] = recs[(size_t)m.f0 + j]; });
      if (in_view && !cov) {
        for (int q = 0; q < n && !cov; ++q) {
          if (outside_box(s_face[q], sx, sy)) continue;
          cov = edges_inside(s_face[q], sx, sy);
        }
      }
      __syncthreads();                                                 // the list is rewritten by the next chunk
    }
    // classify: bit k of `cls` says the pixel counts for entry k
    unsigned cls = 0;
    if (cov) {
      const size_t p = ((size_t)m.view * H + py) * W + px;
      const int mid = mp.mesh_id[p];
      cls = 1u;
      if (mid == it.x) {
        cls |= 2u;
        bool valid = false, scene = false;
        if (mp.sensor) {
          const int raw = mp.sensor[p];
          valid = reading_valid(raw, mp.raw_lo, mp.raw_hi);
          scene = valid && (double)raw * mp.unit < (double)mp.depth[p] - mp.scene_tol_m;
          if (!valid) cls |= 1u << 5;
        }
        const int label = (mp.mask && o.labels) ? o.labels[it.x] : -2;
        if (scene) cls |= 1u << 4;
        else if (label != -2 && !mask_passes(mp.mask[p], label)) cls |= 1u << 6;
        else cls |= 1u << 3;
      } else if (mid >= 0) {
        cls |= 4u;
      } else {
        cls |= 1u << 7;
      }
    }
    for (int k = 0; k < 8; ++k) {
      const unsigned long long b = __ballot((cls >> k) & 1u);
      if (lane == 0 && b) {
        atomicAdd(&s_cnt[k], __popcll(b));
        if (k < 2) {                                                     // amodal, modal: the box of the set lanes
          const int4 bx = ballot_box(b, wave);
          atomicMin(&s_box[k * 4], x0 + bx.x); atomicMin(&s_box[k * 4 + 1], y0 + bx.y);
          atomicMax(&s_box[k * 4 + 2], x0 + bx.z); atomicMax(&s_box[k * 4 + 3], y0 + bx.w);
        }
      }
    }
    __syncthreads();
    if (tid < 8) {
      if (s_cnt[tid]) atomicAdd(&o.counts[(size_t)it.x * 8 + tid], (unsigned long long)s_cnt[tid]);
    } else if (tid < 16) {
      const int k = tid - 8;
      if (s_cnt[k >> 2]) {                                               // coordinates are >= 0: an unsigned min beats the -1
        if (k & 2) atomicMax((int*)&o.boxes[(size_t)it.x * 8 + k], s_box[k]);
        else atomicMin(&o.boxes[(size_t)it.x * 8 + k], (unsigned)s_box[k]);
      }
    }
    __syncthreads();                                                   // s_cnt and s_box are reset by the next item
  }
}

int check_maps(const char* entry, int N, int H, int W, const double* K, double znear, const float* depth, const int32_t* mesh_id,
               const uint16_t* sensor, double unit, int raw_lo, int raw_hi, double scene_tol_m, const uint8_t* mask) {
  if (!K || !depth || !mesh_id) return tile_error(entry, "null pointer");
  if (N < 1 || H < 1 || W < 1 || (long long)N * H * W >= (1ll << 31)) return tile_error(entry, "need N, H, W >= 1 and N H W < 2^31");
  if (!positive_finite(znear)) return tile_error(entry, "znear must be a finite number > 0");
  if (((uintptr_t)depth | (uintptr_t)mesh_id) & 3) return tile_error(entry, "depth and mesh_id must be 4-byte aligned");
  if ((uintptr_t)sensor & 1) return tile_error(entry, "sensor must be 2-byte aligned");
  if (sensor) {
    if (!positive_finite(unit) || !positive_finite(scene_tol_m)) return tile_error(entry, "unit and scene_tol_m must be finite numbers > 0");
    if (raw_lo > raw_hi) return tile_error(entry, "raw_lo > raw_hi");
  }
  return check_cameras(entry, K, N);
}

VisMaps maps_of(int N, int H, int W, const float* depth, const int32_t* mesh_id, const uint16_t* sensor, double unit, int raw_lo,
                int raw_hi, double scene_tol_m, const uint8_t* mask) {
  VisMaps m;
  m.depth = depth; m.mesh_id = mesh_id; m.sensor = sensor; m.mask = mask;
  m.unit = unit; m.scene_tol_m = scene_tol_m; m.raw_lo = raw_lo; m.raw_hi = raw_hi;
  m.N = N; m.H = H; m.W = W;
  return m;
}

}  // namespace

extern "C" int hm_point_visibility(const float* depth, const int32_t* mesh_id, int N, int H, int W, const double* K_host, double znear,
                                   const double* points, int P, const hm_vis_group* groups, int G, int window,
                                   const uint16_t* sensor, double unit, int raw_lo, int raw_hi, double scene_tol_m,
                                   const uint8_t* mask, uint8_t* codes, int32_t* counts, void* stream_) {
  const char* entry = "hm_point_visibility";
  if (G < 0 || P < 0) return tile_error(entry, "negative count");
  if (window < 0 || window > 2) return tile_error(entry, "window must be 0, 1 or 2");
  int rc = check_maps(entry, N, H, W, K_host, znear, depth, mesh_id, sensor, unit, raw_lo, raw_hi, scene_tol_m, mask);
  if (rc != HM_OK) return rc;
  if (G == 0) return HM_OK;
  if (!groups || !counts || (P > 0 && (!points || !codes))) return tile_error(entry, "null pointer");
  if (((uintptr_t)points | (uintptr_t)groups) & 7) return tile_error(entry, "points and groups must be 8-byte aligned");
  if ((uintptr_t)counts & 3) return tile_error(entry, "counts must be 4-byte aligned");
  if ((long long)G * 8 >= (1ll << 31)) return tile_error(entry, "too many groups");
  hipStream_t s = (hipStream_t)stream_;
  HmProfScope prof(HM_K_OTHER, 2, G, P, window, s);
  hipLaunchKernelGGL(vis_counts_init_kernel, dim3((G * 8 + 255) / 256), dim3(256), 0, s, groups, G, P, counts);
  const VisMaps m = maps_of(N, H, W, depth, mesh_id, sensor, unit, raw_lo, raw_hi, scene_tol_m, mask);
  const long long chunks = (long long)(P + 255) / 256 + G;               // non-overlapping ranges: at most this many items
  const int grid = (int)(chunks < 4096 ? chunks : 4096);
  for (int first = 0; first < N; first += VIEWS_PER_LAUNCH) {
    VisCameras cam;
    cam.first = first;
    cam.count = N - first < VIEWS_PER_LAUNCH ? N - first : VIEWS_PER_LAUNCH;
    for (int i = 0; i < cam.count; ++i)
      for (int c = 0; c < 6; ++c) cam.k[i][c] = K_host[(size_t)(first + i) * 9 + c];
    hipLaunchKernelGGL(vis_points_kernel, dim3(grid), dim3(256), 0, s, cam, m, znear, window, points, P, groups, G, codes, counts);
  }
  return hm_check_launch(entry);
}

extern "C" size_t hm_mesh_coverage_workspace_bytes(int N, int H, int W, int n_verts, int n_meshes, int n_faces) {
  if (N <= 0 || H <= 0 || W <= 0 || n_verts < 0 || n_meshes < 0 || n_faces < 0) return 0;
  return layout(H, W, n_meshes, n_faces).total;
}

extern "C" int hm_mesh_coverage(int N, int H, int W, const double* K_host, const double* verts, int n_verts, const int32_t* faces,
                                int n_faces, const hm_mesh* meshes_host, int n_meshes, double znear, const float* depth,
                                const int32_t* mesh_id, const uint16_t* sensor, double unit, int raw_lo, int raw_hi,
                                double scene_tol_m, const uint8_t* mask, const int32_t* labels, int64_t* counts, int32_t* boxes,
                                void* workspace, size_t workspace_bytes, void* stream_) {
  const char* entry = "hm_mesh_coverage";
  if (n_meshes < 0 || n_verts < 0 || n_faces < 0) return tile_error(entry, "negative count");
  int rc = check_maps(entry, N, H, W, K_host, znear, depth, mesh_id, sensor, unit, raw_lo, raw_hi, scene_tol_m, mask);
  if (rc != HM_OK) return rc;
  if (H > 32767 || W > 32767) return tile_error(entry, "need H, W <= 32767");
  if (n_meshes == 0) return HM_OK;
  if (!meshes_host || !counts || !boxes || !workspace) return tile_error(entry, "null pointer");
  if ((n_verts > 0 && !verts) || (n_faces > 0 && !faces)) return tile_error(entry, "null vertices or faces");
  if (((uintptr_t)verts | (uintptr_t)counts | (uintptr_t)workspace) & 7)
    return tile_error(entry, "verts, counts and workspace must be 8-byte aligned");
  if (((uintptr_t)faces | (uintptr_t)boxes | (uintptr_t)labels) & 3) return tile_error(entry, "faces, boxes and labels must be 4-byte aligned");
  rc = check_mesh_table(entry, "view", meshes_host, n_meshes, N, n_verts, n_faces, true);
  if (rc != HM_OK) return rc;
  const TileLayout L = layout(H, W, n_meshes, n_faces);
  if (workspace_bytes < L.total) return tile_error(entry, "workspace too small");
  hipStream_t s = (hipStream_t)stream_;
  char* ws = (char*)workspace;
  HmProfScope prof(HM_K_OTHER, 3, N, H, W, s);
  if (hipMemsetAsync(ws + L.counter, 0, 256, s) != hipSuccess || hipMemsetAsync(counts, 0, (size_t)n_meshes * 8 * sizeof(int64_t), s) != hipSuccess ||
      hipMemsetAsync(boxes, 0xFF, (size_t)n_meshes * 8 * sizeof(int32_t), s) != hipSuccess)
    return hm_set_error(HM_ERR_HIP, "hm_mesh_coverage: hipMemsetAsync");
  for (int first = 0; first < n_meshes; first += MESHES_PER_LAUNCH) {
    MeshBlock mb;
    fill_mesh_block(mb, meshes_host, n_meshes, K_host, first);
    hipLaunchKernelGGL(coverage_setup_kernel, dim3(mb.count), dim3(256), 0, s, mb, verts, faces, H, W, znear, ws, L);
  }
  CoverageOut o;
  o.counts = (unsigned long long*)counts; o.boxes = (unsigned*)boxes; o.labels = labels;
  const VisMaps m = maps_of(N, H, W, depth, mesh_id, sensor, unit, raw_lo, raw_hi, scene_tol_m, mask);
  hipLaunchKernelGGL(coverage_kernel, dim3(raster_grid(n_meshes, H, W)), dim3(256), 0, s, m, o, ws, L);
  return hm_check_launch(entry);
}
