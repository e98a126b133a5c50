// Hand-hand interpenetration: for every query (a, b) the signed distance of every vertex of mesh a to
// the surface of mesh b, with codes, counts and integer sums per query.  The rule is stated in include/hamer_hip.h
// ("Penetration"); tests/penetration_rule.py restates it in numpy.
//  * pen_setup_kernel   - one workgroup per mesh: the vertices in 2^-16 m fixed point (int4: X, Y, Z, valid) and the mesh's
//                integer box and record, into the workspace.  The mesh table travels as kernel arguments, 128 rows per launch.
//  * pen_queries_kernel - the query table (a, b, first output row, first work item) into the workspace, 192 rows per launch.
//  * pen_kernel         - work items are (query, chunk of 64 vertices of a); a workgroup of four waves, every wave holding the
//                same 64 vertices, one lane each.  A query whose boxes are too large or disjoint writes its codes and leaves.
//                Otherwise b's faces are staged 512 at a time in LDS as integer corners in the rule's order with their
//                ownership bits, each wave takes every fourth face (all lanes read one face: a broadcast), and per face a lane
//                makes the crossing test and the fp64 closest-point distance.  The waves' (squared distance, face) minima and
//                parities meet in LDS; wave 0 recomputes the winner's closest point, writes the vertex outputs and sends ballot
//                popcounts and wave sums as one 64-bit integer atomic per term.
// Every coordinate difference the kernel forms is an integer below 2^18 and every product it takes in fp64 an integer below
// 2^53, hence exact; the one larger integer, the plane sign below 2^55, is taken in int64 (the header has the proof).  The
// file is compiled without contraction and every rounded fp64 expression is written in the rule's order.
#include <math.h>
#include "common.h"
#include "raster_tiles.h"

#pragma clang fp contract(off)

namespace {
using raster_tiles::align256;
using raster_tiles::check_mesh_table;
using raster_tiles::tile_error;

constexpr int CHUNK = 64, WAVES = 4, FACE_TILE = 512;
constexpr int MESHES_PER_LAUNCH = 128, QUERIES_PER_LAUNCH = 192;       // argument blocks stay under 4 KiB
constexpr int SIDE_LIMIT = 1 << 17;
constexpr double QUANTA = 65536.0, COORD_LIMIT = 16384.0;
enum { F_OK = 1, F_OWN0 = 2, F_OWN1 = 4, F_OWN2 = 8, F_AREA = 16, F_SOLID = 32 };
enum { S_TESTED = 0, S_NEAR, S_INSIDE, S_INVALID, S_STATUS, S_MAX_BITS, S_SUM_DEPTH, S_PUSH_X, S_PUSH_Y, S_PUSH_Z, S_TERMS };

struct MeshRec { int v0, nv, f0, nf, lo[3], hi[3], n_invalid, pad; };
struct MeshArgs { hm_mesh m[MESHES_PER_LAUNCH]; int count, first; };
struct QueryArgs { int4 q[QUERIES_PER_LAUNCH]; int count, first; };     // a, b, first output row, first work item
struct alignas(16) Face { int x0, y0, z0, x1, y1, z1, x2, y2, z2, flags, pad0, pad1; };
struct Layout { size_t fixed, meshes, queries, total; };

Layout layout(int n_verts, int n_meshes, int n_queries) {
  Layout L;
  L.fixed = 0;
  L.meshes = align256((size_t)n_verts * sizeof(int4));
  L.queries = align256(L.meshes + (size_t)n_meshes * sizeof(MeshRec));
  L.total = align256(L.queries + (size_t)n_queries * sizeof(int4));
  return L;
}

__global__ __launch_bounds__(256) void pen_setup_kernel(MeshArgs ma, const double* __restrict__ verts, int4* __restrict__ fixed,
                                                        MeshRec* __restrict__ recs) {
  __shared__ int s_lo[3], s_hi[3], s_bad;
  const hm_mesh m = ma.m[blockIdx.x];
  const int tid = threadIdx.x;
  if (tid < 3) { s_lo[tid] = INT_MAX; s_hi[tid] = INT_MIN; }
  if (tid == 3) s_bad = 0;
  __syncthreads();
  int lo[3] = {INT_MAX, INT_MAX, INT_MAX}, hi[3] = {INT_MIN, INT_MIN, INT_MIN}, bad = 0;
  for (int i = tid; i < m.nv; i += 256) {
    const double* p = verts + ((size_t)m.v0 + i) * 3;
    const double x = p[0], y = p[1], z = p[2];
    int4 q = make_int4(0, 0, 0, 0);
    if (fabs(x) < COORD_LIMIT && fabs(y) < COORD_LIMIT && fabs(z) < COORD_LIMIT) {       // NaN and inf compare false
      q = make_int4((int)rint(x * QUANTA), (int)rint(y * QUANTA), (int)rint(z * QUANTA), 1);
      lo[0] = min(lo[0], q.x); lo[1] = min(lo[1], q.y); lo[2] = min(lo[2], q.z);
      hi[0] = max(hi[0], q.x); hi[1] = max(hi[1], q.y); hi[2] = max(hi[2], q.z);
    } else {
      ++bad;
    }
    fixed[(size_t)m.v0 + i] = q;
  }
  for (int k = 0; k < 3; ++k) {
    if (lo[k] <= hi[k]) { atomicMin(&s_lo[k], lo[k]); atomicMax(&s_hi[k], hi[k]); }
  }
  if (bad) atomicAdd(&s_bad, bad);
  __syncthreads();
  if (tid == 0) {
    MeshRec r;
    r.v0 = m.v0; r.nv = m.nv; r.f0 = m.f0; r.nf = m.nf;
    for (int k = 0; k < 3; ++k) { r.lo[k] = s_lo[k]; r.hi[k] = s_hi[k]; }
    r.n_invalid = s_bad; r.pad = 0;
    recs[ma.first + blockIdx.x] = r;
  }
}

__global__ __launch_bounds__(256) void pen_queries_kernel(QueryArgs qa, int4* __restrict__ queries) {
  if ((int)threadIdx.x < qa.count) queries[qa.first + threadIdx.x] = qa.q[threadIdx.x];
}

// Edge a -> b owns the samples on its line (hm_mesh_render's top-left rule).
__host__ __device__ __forceinline__ bool owns(int ax, int ay, int bx, int by) {
  const int dy = by - ay, dx = bx - ax;
  return dy < 0 || (dy == 0 && dx > 0);
}

// Face j of mesh b as the rule orders it: flags 0 for a face that names a corner outside the mesh or an invalid vertex (such
// a face is never read further), else the corners with 1 and 2 swapped when the projected area is negative.
__host__ __device__ __forceinline__ Face load_face(const MeshRec& b, int j, const int* __restrict__ faces, const int4* __restrict__ fixed) {
  Face f = {};
  const size_t row = ((size_t)b.f0 + j) * 3;
  const int c0 = faces[row], c1 = faces[row + 1], c2 = faces[row + 2];
  if (c0 < 0 || c0 >= b.nv || c1 < 0 || c1 >= b.nv || c2 < 0 || c2 >= b.nv) return f;     // never read outside the mesh's vertices
  const int4 p0 = fixed[(size_t)b.v0 + c0];
  int4 p1 = fixed[(size_t)b.v0 + c1], p2 = fixed[(size_t)b.v0 + c2];
  if (!(p0.w && p1.w && p2.w)) return f;
  // inside one mesh every difference is below 2^17 (the query is TOO_LARGE otherwise and never comes here)
  long long area = (long long)(p1.x - p0.x) * (p2.y - p0.y) - (long long)(p1.y - p0.y) * (p2.x - p0.x);
  if (area < 0) { const int4 s = p1; p1 = p2; p2 = s; area = -area; }
  const long long abx = p1.x - p0.x, aby = p1.y - p0.y, abz = p1.z - p0.z, acx = p2.x - p0.x, acy = p2.y - p0.y, acz = p2.z - p0.z;
  const bool solid = (aby * acz - abz * acy) != 0 || (abz * acx - abx * acz) != 0 || area != 0;
  f.x0 = p0.x; f.y0 = p0.y; f.z0 = p0.z; f.x1 = p1.x; f.y1 = p1.y; f.z1 = p1.z; f.x2 = p2.x; f.y2 = p2.y; f.z2 = p2.z;
  f.flags = F_OK | (owns(p1.x, p1.y, p2.x, p2.y) ? F_OWN0 : 0) | (owns(p2.x, p2.y, p0.x, p0.y) ? F_OWN1 : 0) |
            (owns(p0.x, p0.y, p1.x, p1.y) ? F_OWN2 : 0) | (area != 0 ? F_AREA : 0) | (solid ? F_SOLID : 0);
  return f;
}

__host__ __device__ __forceinline__ double edge(int ax, int ay, int bx, int by, int px, int py) {      // exact: integers below 2^37
  return (double)(bx - ax) * (double)(py - ay) - (double)(by - ay) * (double)(px - ax);
}
__host__ __device__ __forceinline__ bool covered(double e, int own) { return e > 0.0 || (e == 0.0 && own); }

// Does the ray from (X, Y, Z) in +z cross face f (F_OK and F_AREA set)?
__host__ __device__ __forceinline__ bool crosses(const Face& f, int X, int Y, int Z) {
  if (!covered(edge(f.x1, f.y1, f.x2, f.y2, X, Y), f.flags & F_OWN0) || !covered(edge(f.x2, f.y2, f.x0, f.y0, X, Y), f.flags & F_OWN1) ||
      !covered(edge(f.x0, f.y0, f.x1, f.y1, X, Y), f.flags & F_OWN2))
    return false;
  const long long abx = f.x1 - f.x0, aby = f.y1 - f.y0, abz = f.z1 - f.z0, acx = f.x2 - f.x0, acy = f.y2 - f.y0, acz = f.z2 - f.z0;
  const long long nx = aby * acz - abz * acy, ny = abz * acx - abx * acz, nz = abx * acy - aby * acx;      // |.| < 2^35
  const long long s = nx * (f.x0 - X) + ny * (f.y0 - Y) + nz * (f.z0 - Z);                                 // |.| < 2^55
  return s > 0;
}

// The closest point of face f (F_SOLID set) minus the point, in quanta: the region method in the header's order.  The six
// dot products are integers below 2^38 and exact; what follows them is rounded fp64.
__host__ __device__ __forceinline__ void closest_delta(const Face& f, int X, int Y, int Z, double& dx, double& dy, double& dz) {
  const double abx = f.x1 - f.x0, aby = f.y1 - f.y0, abz = f.z1 - f.z0, acx = f.x2 - f.x0, acy = f.y2 - f.y0, acz = f.z2 - f.z0;
  const double apx = X - f.x0, apy = Y - f.y0, apz = Z - f.z0;
  const double d1 = (abx * apx + aby * apy) + abz * apz, d2 = (acx * apx + acy * apy) + acz * apz;
  if (d1 <= 0.0 && d2 <= 0.0) { dx = -apx; dy = -apy; dz = -apz; return; }
  const double bpx = X - f.x1, bpy = Y - f.y1, bpz = Z - f.z1;
  const double d3 = (abx * bpx + aby * bpy) + abz * bpz, d4 = (acx * bpx + acy * bpy) + acz * bpz;
  if (d3 >= 0.0 && d4 <= d3) { dx = -bpx; dy = -bpy; dz = -bpz; return; }
  const double vc = d1 * d4 - d3 * d2;
  if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) {
    const double v = d1 / (d1 - d3);
    dx = v * abx - apx; dy = v * aby - apy; dz = v * abz - apz;
    return;
  }
  const double cpx = X - f.x2, cpy = Y - f.y2, cpz = Z - f.z2;
  const double d5 = (abx * cpx + aby * cpy) + abz * cpz, d6 = (acx * cpx + acy * cpy) + acz * cpz;
  if (d6 >= 0.0 && d5 <= d6) { dx = -cpx; dy = -cpy; dz = -cpz; return; }
  const double vb = d5 * d2 - d1 * d6;
  if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) {
    const double w = d2 / (d2 - d6);
    dx = w * acx - apx; dy = w * acy - apy; dz = w * acz - apz;
    return;
  }
  const double va = d3 * d6 - d5 * d4;
  if (va <= 0.0 && (d4 - d3) >= 0.0 && (d5 - d6) >= 0.0) {
    const double w = (d4 - d3) / ((d4 - d3) + (d5 - d6));
    dx = w * (double)(f.x2 - f.x1) - bpx; dy = w * (double)(f.y2 - f.y1) - bpy; dz = w * (double)(f.z2 - f.z1) - bpz;
    return;
  }
  const double nx = aby * acz - abz * acy, ny = abz * acx - abx * acz, nz = abx * acy - aby * acx;         // exact
  const double nn = (nx * nx + ny * ny) + nz * nz;
  const double s = (nx * -apx + ny * -apy) + nz * -apz;
  const double t = s / nn;
  dx = nx * t; dy = ny * t; dz = nz * t;
}

__device__ __forceinline__ long long wave_sum(long long v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
  return v;
}
__device__ __forceinline__ unsigned long long wave_max(unsigned long long v) {
  for (int o = 32; o > 0; o >>= 1) { const unsigned long long w = __shfl_down(v, o); v = w > v ? w : v; }
  return v;
}

struct PenOut {
  uint8_t* code;
  float* sdist;
  int32_t* nearest;
  unsigned long long* sums;                        // [n_queries][10], zero on entry
};

__global__ __launch_bounds__(256) void pen_kernel(const int4* __restrict__ fixed, const MeshRec* __restrict__ recs,
                                                  const int4* __restrict__ queries, int n_queries, const int* __restrict__ faces,
                                                  double tol_m, int tol_q, PenOut o) {
  __shared__ Face s_face[FACE_TILE];
  __shared__ double s_d2[WAVES][CHUNK];
  __shared__ int s_best[WAVES][CHUNK];
  __shared__ int s_odd[WAVES][CHUNK];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  // the query of this work item: the last one whose first item is <= blockIdx.x
  int qlo = 0, qhi = n_queries - 1;
  while (qlo < qhi) {
    const int mid = (qlo + qhi + 1) >> 1;
    if (queries[mid].w <= (int)blockIdx.x) qlo = mid; else qhi = mid - 1;
  }
  const int4 q = queries[qlo];
  const int chunk = (int)blockIdx.x - q.w;
  const MeshRec a = recs[q.x], b = recs[q.y];
  unsigned long long* sums = o.sums + (size_t)qlo * S_TERMS;
  const int i = chunk * CHUNK + lane;
  const bool mine = i < a.nv;
  const size_t row = (size_t)q.z + (mine ? i : 0);
  const int4 p = mine ? fixed[(size_t)a.v0 + i] : make_int4(0, 0, 0, 0);

  bool too_large = false, apart = false;
  for (int k = 0; k < 3; ++k) {
    too_large = too_large || (long long)a.hi[k] - a.lo[k] >= SIDE_LIMIT || (long long)b.hi[k] - b.lo[k] >= SIDE_LIMIT;
    apart = apart || !((long long)a.lo[k] <= (long long)b.hi[k] + tol_q && (long long)b.lo[k] - tol_q <= (long long)a.hi[k]);
  }
  if (too_large || apart) {                                              // nothing is staged
    if (wave == 0) {
      if (mine) {
        const bool bad = too_large || !p.w;
        o.code[row] = bad ? HM_PEN_INVALID : HM_PEN_FAR;
        o.sdist[row] = bad ? __builtin_nanf("") : __builtin_inff();
        o.nearest[row] = -1;
      }
      if (chunk == 0 && lane == 0) {
        sums[S_STATUS] = too_large ? HM_PEN_TOO_LARGE : HM_PEN_DISJOINT;
        if (!too_large && a.n_invalid) sums[S_INVALID] = (unsigned long long)a.n_invalid;
      }
    }
    return;
  }
  // inside b's box inflated by the tolerance: every difference to a vertex of b is below 2^17 + 2^16
  const bool tested = mine && p.w && p.x >= b.lo[0] - tol_q && p.x <= b.hi[0] + tol_q && p.y >= b.lo[1] - tol_q &&
                      p.y <= b.hi[1] + tol_q && p.z >= b.lo[2] - tol_q && p.z <= b.hi[2] + tol_q;
  double best_d2 = __builtin_inf();
  int best = -1, odd = 0;
  if (__ballot(tested)) {                                                // the same in all four waves
    for (int t0 = 0; t0 < b.nf; t0 += FACE_TILE) {
      const int n = min(FACE_TILE, b.nf - t0);
      for (int j = tid; j < n; j += 256) s_face[j] = load_face(b, t0 + j, faces, fixed);
      __syncthreads();
      for (int j = wave; j < n; j += WAVES) {
        const Face f = s_face[j];
        if (!(f.flags & F_OK) || !tested) continue;
        if ((f.flags & F_AREA) && crosses(f, p.x, p.y, p.z)) odd ^= 1;
        if (f.flags & F_SOLID) {
          double dx, dy, dz;
          closest_delta(f, p.x, p.y, p.z, dx, dy, dz);
          const double d2 = (dx * dx + dy * dy) + dz * dz;
          if (d2 < best_d2) { best_d2 = d2; best = t0 + j; }
        }
      }
      __syncthreads();                                                   // the tile is rewritten by the next round
    }
  }
  s_d2[wave][lane] = best_d2; s_best[wave][lane] = best; s_odd[wave][lane] = odd;
  __syncthreads();
  if (wave != 0) return;
  for (int w = 1; w < WAVES; ++w) {
    const double d2 = s_d2[w][lane];
    const int bj = s_best[w][lane];
    odd ^= s_odd[w][lane];
    if (bj >= 0 && (d2 < best_d2 || (d2 == best_d2 && bj < best))) { best_d2 = d2; best = bj; }
  }
  int code = p.w ? HM_PEN_FAR : HM_PEN_INVALID;
  float sd = p.w ? __builtin_inff() : __builtin_nanf("");
  int nearest = -1;
  long long depth_q = 0, px = 0, py = 0, pz = 0;
  unsigned long long bits = 0;
  if (tested && best >= 0) {
    const double d = sqrt(best_d2) * (1.0 / QUANTA);                     // metres
    if (odd) {
      const Face f = load_face(b, best, faces, fixed);
      double dx, dy, dz;
      closest_delta(f, p.x, p.y, p.z, dx, dy, dz);
      code = HM_PEN_INSIDE; sd = (float)-d; nearest = best;
      bits = (unsigned long long)__double_as_longlong(d);
      depth_q = (long long)rint(d * 4294967296.0);
      px = (long long)rint(dx * QUANTA); py = (long long)rint(dy * QUANTA); pz = (long long)rint(dz * QUANTA);
    } else if (d <= tol_m) {
      code = HM_PEN_NEAR; sd = (float)d; nearest = best;
    }
  }
  if (mine) { o.code[row] = (uint8_t)code; o.sdist[row] = sd; o.nearest[row] = nearest; }
  const int n_tested = __popcll(__ballot(tested)), n_near = __popcll(__ballot(mine && code == HM_PEN_NEAR));
  const int n_inside = __popcll(__ballot(mine && code == HM_PEN_INSIDE)), n_invalid = __popcll(__ballot(mine && code == HM_PEN_INVALID));
  if (n_inside) {                                                        // uniform
    depth_q = wave_sum(depth_q); px = wave_sum(px); py = wave_sum(py); pz = wave_sum(pz);
    bits = wave_max(bits);
  }
  if (lane == 0) {
    if (n_tested) atomicAdd(&sums[S_TESTED], (unsigned long long)n_tested);
    if (n_near) atomicAdd(&sums[S_NEAR], (unsigned long long)n_near);
    if (n_invalid) atomicAdd(&sums[S_INVALID], (unsigned long long)n_invalid);
    if (n_inside) {
      atomicAdd(&sums[S_INSIDE], (unsigned long long)n_inside);
      atomicMax(&sums[S_MAX_BITS], bits);
      atomicAdd(&sums[S_SUM_DEPTH], (unsigned long long)depth_q);
      atomicAdd(&sums[S_PUSH_X], (unsigned long long)px);                // two's complement: the signed sum
      atomicAdd(&sums[S_PUSH_Y], (unsigned long long)py);
      atomicAdd(&sums[S_PUSH_Z], (unsigned long long)pz);
    }
  }
}

bool items_of(const hm_mesh* meshes, const hm_pen_query* queries, int n_queries, long long& rows, long long& items) {
  rows = items = 0;
  for (int q = 0; q < n_queries; ++q) {
    const int nv = meshes[queries[q].a].nv;
    rows += nv;
    items += nv > 0 ? (nv + CHUNK - 1) / CHUNK : 1;                      // a query without vertices still reports its status
  }
  return rows < (1ll << 31) && items < (1ll << 31);
}

}  // namespace

extern "C" size_t hm_mesh_penetration_workspace_bytes(int n_verts, int n_meshes, int n_queries) {
  if (n_verts < 0 || n_meshes < 0 || n_queries < 0) return 0;
  return layout(n_verts, n_meshes, n_queries).total;
}

extern "C" int hm_mesh_penetration(const double* verts, int n_verts, const int32_t* faces, int n_faces, const hm_mesh* meshes_host,
                                   int n_meshes, const hm_pen_query* queries_host, int n_queries, double contact_tol_m,
                                   uint8_t* code, float* signed_distance, int32_t* nearest_face, long long n_rows, int64_t* sums,
                                   void* workspace, size_t workspace_bytes, void* stream_) {
  const char* entry = "hm_mesh_penetration";
  if (n_meshes < 0 || n_verts < 0 || n_faces < 0 || n_queries < 0 || n_rows < 0) return tile_error(entry, "negative count");
  if (!(contact_tol_m >= 0.0 && contact_tol_m <= 1.0)) return tile_error(entry, "contact_tol_m must lie in 0 .. 1 m");
  if (n_queries == 0) return HM_OK;
  if (!meshes_host || !queries_host || !sums || !workspace) return tile_error(entry, "null pointer");
  if ((n_verts > 0 && !verts) || (n_faces > 0 && !faces)) return tile_error(entry, "null vertices or faces");
  if (((uintptr_t)verts | (uintptr_t)sums) & 7) return tile_error(entry, "verts and sums must be 8-byte aligned");
  if ((uintptr_t)workspace & 15) return tile_error(entry, "workspace must be 16-byte aligned");
  if (((uintptr_t)faces | (uintptr_t)signed_distance | (uintptr_t)nearest_face) & 3)
    return tile_error(entry, "faces, signed_distance and nearest_face must be 4-byte aligned");
  int rc = check_mesh_table(entry, "frame", meshes_host, n_meshes, INT_MAX, n_verts, n_faces, true);
  if (rc != HM_OK) return rc;
  for (int q = 0; q < n_queries; ++q)
    if (queries_host[q].a < 0 || queries_host[q].a >= n_meshes || queries_host[q].b < 0 || queries_host[q].b >= n_meshes)
      return tile_error(entry, "a query names a mesh outside the table");
  long long rows, items;
  if (!items_of(meshes_host, queries_host, n_queries, rows, items)) return tile_error(entry, "too many vertex rows or work items");
  if (rows > n_rows) return tile_error(entry, "n_rows is smaller than the queries' vertex count");
  if (rows > 0 && (!code || !signed_distance || !nearest_face)) return tile_error(entry, "null output");
  const Layout L = layout(n_verts, n_meshes, n_queries);
  if (workspace_bytes < L.total) return tile_error(entry, "workspace too small");
  hipStream_t s = (hipStream_t)stream_;
  char* ws = (char*)workspace;
  int4* fixed = (int4*)(ws + L.fixed);
  MeshRec* recs = (MeshRec*)(ws + L.meshes);
  int4* qtab = (int4*)(ws + L.queries);
  HmProfScope prof(HM_K_OTHER, 4, n_queries, n_meshes, (int)rows, s);
  if (hipMemsetAsync(sums, 0, (size_t)n_queries * S_TERMS * sizeof(int64_t), s) != hipSuccess)
    return hm_set_error(HM_ERR_HIP, "hm_mesh_penetration: hipMemsetAsync");
  for (int first = 0; first < n_meshes; first += MESHES_PER_LAUNCH) {
    MeshArgs ma;
    ma.first = first;
    ma.count = n_meshes - first < MESHES_PER_LAUNCH ? n_meshes - first : MESHES_PER_LAUNCH;
    for (int i = 0; i < ma.count; ++i) ma.m[i] = meshes_host[first + i];
    hipLaunchKernelGGL(pen_setup_kernel, dim3(ma.count), dim3(256), 0, s, ma, verts, fixed, recs);
  }
  long long row0 = 0, item0 = 0;
  for (int first = 0; first < n_queries; first += QUERIES_PER_LAUNCH) {
    QueryArgs qa;
    qa.first = first;
    qa.count = n_queries - first < QUERIES_PER_LAUNCH ? n_queries - first : QUERIES_PER_LAUNCH;
    for (int i = 0; i < qa.count; ++i) {
      const hm_pen_query& q = queries_host[first + i];
      const int nv = meshes_host[q.a].nv;
      qa.q[i] = make_int4(q.a, q.b, (int)row0, (int)item0);
      row0 += nv;
      item0 += nv > 0 ? (nv + CHUNK - 1) / CHUNK : 1;
    }
    hipLaunchKernelGGL(pen_queries_kernel, dim3(1), dim3(256), 0, s, qa, qtab);
  }
  PenOut o;
  o.code = code; o.sdist = signed_distance; o.nearest = nearest_face; o.sums = (unsigned long long*)sums;
  const int tol_q = (int)ceil(contact_tol_m * QUANTA);
  hipLaunchKernelGGL(pen_kernel, dim3((unsigned)items), dim3(256), 0, s, fixed, recs, qtab, n_queries, faces, contact_tol_m, tol_q, o);
  return hm_check_launch(entry);
}
