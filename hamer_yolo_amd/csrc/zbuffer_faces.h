// The z-buffer face rule (include/hamer_hip.h, hm_mesh_render), shared by zrender.hip and
// visibility.hip: which pixel centres a face covers.  A mesh's modal pixel count (hm_mesh_coverage) equals the number of pixels
// the renderer labels with it only because both evaluate ONE statement of this rule: the fp64 projection to 24.8 fixed point,
// the validity tests, the winding swap, the top-left ownership bits, the pixel box and the integer edge functions at the
// pixel centre (int32 when the face's box spans less than 2^15 sub-pixel units, int64 otherwise).
// Unlike raster_tiles.h, whose header comment keeps every fp expression of a rule in the rule's own file, this header does hold
// one: the projection.  Both users and the point kernel need its bits equal, so it is written once, here, and the header
// therefore sets contraction off itself, at file scope, before anything else; the pragma stays in force in the including file.
// Every expression keeps the order written in include/hamer_hip.h.  The "finite number > 0" test of the argument checks is not
// here but in hamer_hip_internal.h (positive_finite): the depth units and mask_fit.hip make it too and do not draw.
#pragma once
#pragma clang fp contract(off)
#include "raster_tiles.h"

namespace zbuffer_faces {
using namespace raster_tiles;

constexpr int MESHES_PER_LAUNCH = 48;              // kernel argument block stays under 4 KiB
constexpr int F_SMALL = 1, F_OWN0 = 2, F_OWN1 = 4, F_OWN2 = 8;

// What every face record begins with, or is.  Corners are in the order the rule leaves them (1 and 2 swapped when the signed
// area was negative), in 24.8 fixed point; all zero for a face the rule drops.  `tag` is the user's: the renderer's mesh row
// or the face's index in its mesh; the rule never reads it.  32 bytes, aligned like the records that start with it, so a
// copy moves whole 16-byte pieces.
struct alignas(8) FaceGeom { int x0, y0, x1, y1, x2, y2, flags, tag; };
// What the renderer keeps beyond that: the corners' indices inside the mesh and 1 / z, in the swapped order, and twice the
// area (> 0, exact).
struct FaceRest { int c0, c1, c2; double r0, r1, r2, area2; };

struct MeshEntry {
  hm_mesh m;
  double k[6];                                     // K00 K01 K02 K10 K11 K12 of the mesh's view
};
struct MeshBlock {
  MeshEntry m[MESHES_PER_LAUNCH];
  int count, first;
};

// Camera-frame (x, y, z), z >= znear tested by the caller, to 24.8 fixed point; false when a coordinate leaves (-65536, 65536).
__device__ __forceinline__ bool project_fixed(const double* k, double x, double y, double z, int& X, int& Y) {
  const double u = ((k[0] * x + k[1] * y) + k[2] * z) / z;
  const double v = ((k[3] * x + k[4] * y) + k[5] * z) / z;
  if (!(fabs(u) < 65536.0) || !(fabs(v) < 65536.0)) return false;
  X = (int)rint(256.0 * u); Y = (int)rint(256.0 * v);                  // |.| <= 2^24
  return true;
}

// Edge a -> b owns the samples on its line: a top edge or a left edge of a triangle of positive area.
__device__ __forceinline__ bool owns(int ax, int ay, int bx, int by) {
  const int dy = by - ay, dx = bx - ax;
  return dy < 0 || (dy == 0 && dx > 0);
}
__device__ __forceinline__ bool covered(long long e, bool own) { return e > 0 || (e == 0 && own); }

// The face loop of a setup kernel (one workgroup of 256 lanes per mesh): per face the corners, the validity tests, the swap,
// the area, the flags and the pixel box clipped to the view.  The caller's record, all zero for a face the rule drops and
// else filled by fill(record, geometry, rest), goes to `recs`, the box to `boxes`.  Returns the box of the lane's faces for
// emit_mesh_tiles (left, top, right, bottom; empty when left > right).
template <class Rec, class Fill>
__device__ __forceinline__ int4 setup_faces(const MeshEntry& e, const double* __restrict__ verts, const int* __restrict__ faces, int H,
                                            int W, double znear, Rec* __restrict__ recs, int4* __restrict__ boxes, Fill&& fill) {
  const hm_mesh m = e.m;
  const double k[6] = {e.k[0], e.k[1], e.k[2], e.k[3], e.k[4], e.k[5]};
  const double* vb = verts + (size_t)m.v0 * 3;
  int4 mine = make_int4(INT_MAX, INT_MAX, INT_MIN, INT_MIN);
  for (int j = threadIdx.x; j < m.nf; j += 256) {
    const size_t fid = (size_t)m.f0 + j;
    int c[3] = {faces[fid * 3], faces[fid * 3 + 1], faces[fid * 3 + 2]};
    bool ok = true;
    int X[3] = {0, 0, 0}, Y[3] = {0, 0, 0};
    double R[3] = {0, 0, 0};
    for (int q = 0; q < 3; ++q) {
      if (c[q] < 0 || c[q] >= m.nv) { ok = false; continue; }         // never read outside the mesh's vertices
      const double x = vb[(size_t)c[q] * 3], y = vb[(size_t)c[q] * 3 + 1], z = vb[(size_t)c[q] * 3 + 2];
      int px = 0, py = 0;
      const bool in_range = project_fixed(k, x, y, z, px, py);
      if (!(z >= znear) || !in_range) { ok = false; continue; }
      X[q] = px; Y[q] = py;
      R[q] = 1.0 / z;
    }
    int4 box = make_int4(1, 1, 0, 0);                                  // empty
    Rec r = {};
    if (ok) {
      long long area = edge64(X[0], Y[0], X[1], Y[1], X[2], Y[2]);
      if (area < 0) {
        int s = X[1]; X[1] = X[2]; X[2] = s;
        s = Y[1]; Y[1] = Y[2]; Y[2] = s;
        s = c[1]; c[1] = c[2]; c[2] = s;
        const double d = R[1]; R[1] = R[2]; R[2] = d;
        area = -area;
      }
      if (area != 0) {
        const int fx0 = min(X[0], min(X[1], X[2])), fx1 = max(X[0], max(X[1], X[2]));
        const int fy0 = min(Y[0], min(Y[1], Y[2])), fy1 = max(Y[0], max(Y[1], Y[2]));
        // E_i is the edge function of the edge opposite corner i: 1 -> 2, 2 -> 0, 0 -> 1
        const int flags = ((fx1 - fx0) < 32768 && (fy1 - fy0) < 32768 ? F_SMALL : 0) | (owns(X[1], Y[1], X[2], Y[2]) ? F_OWN0 : 0) |
                          (owns(X[2], Y[2], X[0], Y[0]) ? F_OWN1 : 0) | (owns(X[0], Y[0], X[1], Y[1]) ? F_OWN2 : 0);
        fill(r, FaceGeom{X[0], Y[0], X[1], Y[1], X[2], Y[2], flags, 0}, FaceRest{c[0], c[1], c[2], R[0], R[1], R[2], (double)area});
        // pixels whose centre 256 p + 128 lies inside the corners' box (arithmetic shifts: floor), clipped to the view
        box = make_int4(max((fx0 + 127) >> 8, 0), max((fy0 + 127) >> 8, 0), min((fx1 - 128) >> 8, W - 1), min((fy1 - 128) >> 8, H - 1));
        if (box.x <= box.z && box.y <= box.w) {
          mine.x = min(mine.x, box.x); mine.y = min(mine.y, box.y); mine.z = max(mine.z, box.z); mine.w = max(mine.w, box.w);
        } else {
          box = make_int4(1, 1, 0, 0);
        }
      }
    }
    recs[fid] = r;
    boxes[fid] = box;
  }
  return mine;
}

// The sample test, in two steps so that a caller's loop can `continue` after either: is the sample (sx, sy), a pixel centre
// in 24.8 fixed point, outside the corners' box?  Inside the box every difference is < the span.
__device__ __forceinline__ bool outside_box(const FaceGeom& f, int sx, int sy) {
  const int fx0 = min(f.x0, min(f.x1, f.x2)), fx1 = max(f.x0, max(f.x1, f.x2));
  const int fy0 = min(f.y0, min(f.y1, f.y2)), fy1 = max(f.y0, max(f.y1, f.y2));
  return sx < fx0 || sx > fx1 || sy < fy0 || sy > fy1;
}
// Does face f cover a sample inside its box?  e0..e2: the edge values (E_0, E_1, E_2), exact as doubles; the renderer's depth
// is made of them.
__device__ __forceinline__ bool edges_inside(const FaceGeom& f, int sx, int sy, double& e0, double& e1, double& e2) {
  bool in;
  if (f.flags & F_SMALL) {                                             // |e| < 2^31: two products below 2^30
    const int a = edge32(f.x1, f.y1, f.x2, f.y2, sx, sy), b = edge32(f.x2, f.y2, f.x0, f.y0, sx, sy),
              c = edge32(f.x0, f.y0, f.x1, f.y1, sx, sy);
    in = covered(a, f.flags & F_OWN0) && covered(b, f.flags & F_OWN1) && covered(c, f.flags & F_OWN2);
    e0 = (double)a; e1 = (double)b; e2 = (double)c;
  } else {
    const long long a = edge64(f.x1, f.y1, f.x2, f.y2, sx, sy), b = edge64(f.x2, f.y2, f.x0, f.y0, sx, sy),
                    c = edge64(f.x0, f.y0, f.x1, f.y1, sx, sy);
    in = covered(a, f.flags & F_OWN0) && covered(b, f.flags & F_OWN1) && covered(c, f.flags & F_OWN2);
    e0 = (double)a; e1 = (double)b; e2 = (double)c;
  }
  return in;
}
__device__ __forceinline__ bool edges_inside(const FaceGeom& f, int sx, int sy) {
  double e0, e1, e2;
  return edges_inside(f, sx, sy, e0, e1, e2);
}

// ---------------------------------------------------------------------------------------------------------------- host side
// Block `first` of the mesh table with each mesh's camera; returns the largest vertex count among its meshes.
inline int fill_mesh_block(MeshBlock& mb, const hm_mesh* meshes, int n_meshes, const double* K, int first) {
  mb.first = first;
  mb.count = n_meshes - first < MESHES_PER_LAUNCH ? n_meshes - first : MESHES_PER_LAUNCH;
  int max_nv = 0;
  for (int i = 0; i < mb.count; ++i) {
    mb.m[i].m = meshes[first + i];
    for (int c = 0; c < 6; ++c) mb.m[i].k[c] = K[(size_t)mb.m[i].m.frame * 9 + c];
    max_nv = mb.m[i].m.nv > max_nv ? mb.m[i].m.nv : max_nv;
  }
  return max_nv;
}

inline int check_cameras(const char* entry, const double* K, int N) {
  for (int n = 0; n < N; ++n)
    if (!(K[n * 9 + 6] == 0.0 && K[n * 9 + 7] == 0.0 && K[n * 9 + 8] == 1.0))
      return tile_error(entry, "the last row of every K must be exactly (0, 0, 1)");
  return HM_OK;
}

}  // namespace zbuffer_faces
