// The tile-binning core of the drawing path, shared by render.hip, zrender.hip and skeleton.hip: a
// setup kernel cuts each mesh's clipped box into 16 x 16 tiles and appends them to a work list through one atomic counter, a
// raster kernel walks the list with one lane per pixel, culling the mesh's faces against the tile into LDS, and sends the
// winning 64-bit key to the view's key buffer; a last pass takes the keys and leaves the buffer as it found it.
// Nothing in this header does floating-point arithmetic that could be contracted (rint_u8 only rounds and compares).  Every
// fp32 / fp64 expression of a drawing rule -- projection, depth, shading, blend -- stays in its own file under that file's
// `#pragma clang fp contract(off)`, which is what keeps the bytes equal to the numpy rules (zbuffer_faces.h, which builds on
// this header, holds the one projection two files share and says why).
// The skeleton kernels use TILE, align256, the item packing and the tile-overlap predicate only: their per-tile flag claim
// and their one-wave cull are different algorithms.
#pragma once
#include <limits.h>
#include <math.h>
#include <algorithm>
#include <numeric>
#include <string>
#include <vector>
#include "hamer_hip_internal.h"

namespace raster_tiles {

constexpr int TILE = 16;
constexpr unsigned long long NO_KEY = ~0ull;       // the key buffer holds this between calls (0xFF bytes)

inline size_t align256(size_t x) { return (x + 255) & ~size_t(255); }
inline size_t tiles_of(int H, int W) { return (size_t)((H + TILE - 1) / TILE) * ((W + TILE - 1) / TILE); }

// A work item is (list owner, tile): the tile's row and column in one int (H, W <= 32767, so both are below 2^11).
__device__ __forceinline__ int pack_tile(int tx, int ty) { return (ty << 16) | tx; }
__device__ __forceinline__ int tile_x(int packed) { return packed & 0xFFFF; }
__device__ __forceinline__ int tile_y(int packed) { return packed >> 16; }
// The flag byte of tile (tx, ty) of a view.
__device__ __forceinline__ size_t tile_index(int view, int tx, int ty, int H, int W) {
  const int tiles_x = (W + TILE - 1) / TILE, tiles = tiles_x * ((H + TILE - 1) / TILE);
  return (size_t)view * tiles + ty * tiles_x + tx;
}

// Does the pixel box b = (left, top, right, bottom), inclusive and empty when left > right, meet the tile whose first
// pixel is (x0, y0)?
__device__ __forceinline__ bool box_meets_tile(int4 b, int x0, int y0) {
  return b.x <= b.z && b.x <= x0 + TILE - 1 && b.z >= x0 && b.y <= y0 + TILE - 1 && b.w >= y0;
}

// Edge function of a -> b at p: exact in int64 always, in int32 where the caller knows both products stay below 2^30.
__device__ __forceinline__ long long edge64(int ax, int ay, int bx, int by, int px, int py) {
  return (long long)(bx - ax) * (py - ay) - (long long)(by - ay) * (px - ax);
}
__device__ __forceinline__ int edge32(int ax, int ay, int bx, int by, int px, int py) {
  return (bx - ax) * (py - ay) - (by - ay) * (px - ax);
}

__device__ __forceinline__ unsigned rint_u8(double v) {
  const double r = rint(v);
  return !(r >= 0.0) ? 0u : (r > 255.0 ? 255u : (unsigned)r);          // not-a-number -> 0
}

// Workspace of the two mesh renderers.  Everything up to `boxes` is the same arithmetic for both; `tail` is the one array
// a renderer adds (render.hip: a colour per face, zrender.hip: a normal per vertex).
struct TileLayout {
  size_t keys, counter, flags, meshes, items, recs, boxes, tail, total;
};
struct MeshRec { int view, f0, nf, pad; };         // what raster needs of a mesh

inline TileLayout tile_layout(int N, int H, int W, int n_meshes, int n_faces, size_t face_rec_bytes, size_t tail_bytes) {
  const size_t tiles = tiles_of(H, W);
  TileLayout L;
  L.keys = 0;                                                          // N*H*W keys, first: their place never moves
  L.counter = align256((size_t)N * H * W * 8);
  L.flags = L.counter + 256;                                           // one byte per (view, tile): a key was written there
  L.meshes = align256(L.flags + (size_t)N * tiles);
  L.items = align256(L.meshes + (size_t)n_meshes * sizeof(MeshRec));
  L.recs = align256(L.items + (size_t)n_meshes * tiles * sizeof(int2));
  L.boxes = align256(L.recs + (size_t)n_faces * face_rec_bytes);
  L.tail = align256(L.boxes + (size_t)n_faces * sizeof(int4));
  L.total = align256(L.tail + tail_bytes);
  return L;
}

// The end of a setup kernel (one workgroup of 256 lanes per mesh): each lane brings the box of its faces (empty when
// lx0 > lx1); the mesh's box is cut into tiles, one atomicAdd reserves their slots on the work list, and the mesh record
// and the items are written.  Called by every lane of the workgroup.
__device__ __forceinline__ void emit_mesh_tiles(int lx0, int ly0, int lx1, int ly1, int mesh, MeshRec rec, char* __restrict__ ws,
                                                const TileLayout& L) {
  __shared__ int bx0, by0, bx1, by1, base;
  const int tid = threadIdx.x;
  if (tid == 0) { bx0 = INT_MAX; by0 = INT_MAX; bx1 = INT_MIN; by1 = INT_MIN; }
  __syncthreads();
  if (lx0 <= lx1) { atomicMin(&bx0, lx0); atomicMin(&by0, ly0); atomicMax(&bx1, lx1); atomicMax(&by1, ly1); }
  __syncthreads();
  const bool any = bx0 <= bx1;
  const int tx0 = any ? bx0 / TILE : 0, ty0 = any ? by0 / TILE : 0;
  const int ntx = any ? bx1 / TILE - tx0 + 1 : 0, nty = any ? by1 / TILE - ty0 + 1 : 0;
  if (tid == 0) {
    base = ntx * nty ? (int)atomicAdd((unsigned*)(ws + L.counter), (unsigned)(ntx * nty)) : 0;
    ((MeshRec*)(ws + L.meshes))[mesh] = rec;
  }
  __syncthreads();
  int2* items = (int2*)(ws + L.items);
  for (int t = tid; t < ntx * nty; t += 256)
    items[base + t] = make_int2(mesh, pack_tile(tx0 + t % ntx, ty0 + t / ntx));
}

// The cull step of a raster kernel (256 lanes): the lanes with `hit` get consecutive slots 0 .. n - 1 in lane order
// (ballot inside a wave, a prefix over the four waves' counts) and each calls write_record(slot) to fill the LDS list.
// Returns n to every lane; the list is complete on return.  Two barriers; the caller adds one after it has read the list,
// before the next call rewrites it.
template <class WriteRecord>
__device__ __forceinline__ int cull_to_lds(bool hit, WriteRecord&& write_record) {
  __shared__ int s_wave[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long mask = __ballot(hit);
  const int before = __popcll(mask & ((1ull << lane) - 1));
  if (lane == 0) s_wave[wave] = __popcll(mask);
  __syncthreads();
  int off = 0, n = 0;
  for (int q = 0; q < 4; ++q) { off += q < wave ? s_wave[q] : 0; n += s_wave[q]; }
  if (hit) write_record(off + before);
  __syncthreads();
  return n;
}

// A pixel's winning key goes to the view's key buffer, and the tile's flag says that the tile holds keys.
__device__ __forceinline__ void commit_key(char* __restrict__ ws, const TileLayout& L, size_t pixel, size_t tile,
                                           unsigned long long key) {
  atomicMin((unsigned long long*)(ws + L.keys) + pixel, key);
  ((unsigned char*)(ws + L.flags))[tile] = 1;
}

// The key of a pixel, taken: keys are read in flagged tiles only, and a key that was set is reset on the way, so the key
// buffer is NO_KEY everywhere on return, as it was on entry.  Both renderers may therefore share one buffer call after call.
__device__ __forceinline__ unsigned long long take_key(char* __restrict__ ws, const TileLayout& L, size_t pixel, size_t tile) {
  if (!((const unsigned char*)(ws + L.flags))[tile]) return NO_KEY;
  unsigned long long* kp = (unsigned long long*)(ws + L.keys) + pixel;
  const unsigned long long key = *kp;
  if (key != NO_KEY) *kp = NO_KEY;
  return key;
}

// ---------------------------------------------------------------------------------------------------------------- host side
inline int tile_error(const char* entry, const std::string& what) { return hm_set_error(HM_ERR_ARG, (std::string(entry) + ": " + what).c_str()); }

// The mesh table of a call: every mesh in a view of the batch, its ranges inside the arrays, no face row shared by two
// meshes (a face id names one face of one mesh) and, if asked, no vertex row either (a vertex row carries one normal).
// `noun` is what the entry point calls hm_mesh.frame: "frame" or "view".
inline int check_mesh_table(const char* entry, const char* noun, const hm_mesh* meshes, int n_meshes, int N, int n_verts, int n_faces,
                            bool verts_disjoint) {
  for (int i = 0; i < n_meshes; ++i) {
    const hm_mesh& m = meshes[i];
    if (m.frame < 0 || m.frame >= N) return tile_error(entry, std::string("mesh ") + noun + " outside the batch");
    if (m.nv < 0 || m.nf < 0 || m.v0 < 0 || m.f0 < 0) return tile_error(entry, "negative mesh range");
    if (m.nv == 0 && m.nf > 0) return tile_error(entry, "a mesh with faces but no vertices");
    if ((long long)m.v0 + m.nv > n_verts || (long long)m.f0 + m.nf > n_faces)
      return tile_error(entry, "mesh range outside the vertex or face array");
  }
  // sorted by their first row, overlapping ranges are neighbours
  std::vector<int> order(n_meshes);
  std::iota(order.begin(), order.end(), 0);
  auto overlap = [&](int32_t hm_mesh::*first, int32_t hm_mesh::*count) {
    std::sort(order.begin(), order.end(), [&](int a, int b) { return meshes[a].*first < meshes[b].*first; });
    long long end = 0;
    for (int i : order) {
      if (meshes[i].*count == 0) continue;
      if (meshes[i].*first < end) return true;
      end = (long long)(meshes[i].*first) + meshes[i].*count;
    }
    return false;
  };
  if (overlap(&hm_mesh::f0, &hm_mesh::nf)) return tile_error(entry, "two meshes share faces");
  if (verts_disjoint && overlap(&hm_mesh::v0, &hm_mesh::nv)) return tile_error(entry, "two meshes share vertices");
  return HM_OK;
}

// `out` is never `frames` drawn in place: the two arrays of `bytes` bytes must not overlap.
inline int check_out_apart(const char* entry, const uint8_t* frames, const uint8_t* out, size_t bytes) {
  if (frames && out && frames < out + bytes && out < frames + bytes) return tile_error(entry, "out overlaps frames (never in place)");
  return HM_OK;
}

// Workgroups of a raster launch: one per possible work item (`lists` lists of at most every tile of a view), at most `cap`.
inline int raster_grid(size_t lists, int H, int W, size_t cap = 2048) { return (int)std::min(lists * tiles_of(H, W), cap); }

}  // namespace raster_tiles
