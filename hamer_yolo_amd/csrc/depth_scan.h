// The covered-pixel scan core of the depth path, shared by depth_eval.hip and depth_fit.hip: ONE pass
// over the N * H * W values of the z-buffer's pred_id for all queries, the integer gate every covered pixel goes through, the
// per-workgroup query slots, the grouping of a wave's 64 pixels by query, and the host checks of the arguments both entry points
// take.  What a kernel adds up per query, and where, is its own: the body it passes to for_each_query.  The walk: the pixels are
// read as consecutive int32 of pred_id, not row by row.  From the first 16-byte aligned address on, a thread reads UNROLL 16-byte
// vectors per round (load_round issues all of them before the caller looks at any) and a workgroup of THREADS threads does ROUNDS
// rounds, 32768 pixels; the up to 3 pixels before that address and behind the last whole vector are read one by one by the first
// wave of workgroup 0 (scan_edges).  A vector of four -1 -- nearly all -- costs that load: no other map is read for its pixels.
// Nothing in this header does fp32 / fp64 arithmetic of a rule, and nothing may: the gate compares integers.  Every expression
// of a rule -- residual, bin, normal, the 28 terms -- stays in its own file under that file's `#pragma clang fp contract(off)`,
// which is what keeps the integers equal to the numpy rules.
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include "hamer_hip_internal.h"

namespace depth_scan {

constexpr int THREADS = 256, UNROLL = 4, ROUNDS = 8;
constexpr long long VECS = (long long)THREADS * UNROLL * ROUNDS;        // 16-byte vectors per workgroup: 32768 pixels
// The first three counts of a query, and MEASURED: the stage of a pixel that passed the gate, where a kernel's own counts begin.
enum { COVERED = 0, OFF_MASK = 1, NO_MEASUREMENT = 2, MEASURED = 3 };

// The map inputs of both kernels (include/hamer_hip.h, "Depth residuals"); a kernel's parameters derive from this.
struct Maps {
  const float* depth; const int32_t* id; const uint16_t* sensor; const uint8_t* mask; const int32_t* labels;
  const int32_t* mesh_query; long long total;             // total: N * H * W, below 2^31 (host_checks sets it)
  int n_meshes, Q, raw_lo, raw_hi; double unit;
};

// head: the pixels before the first aligned address (0..3, at most total); nvec: the whole vectors from there on, based at vec;
// tail0: the first pixel behind the last whole vector (total - tail0 is 0..3).
struct Walk { long long total, head, nvec, tail0; const int4* vec; };
__device__ __forceinline__ Walk walk_of(const int32_t* id, long long total) {
  long long head = (long long)((16u - (unsigned)((uintptr_t)id & 15u)) & 15u) >> 2;
  if (head > total) head = total;
  const long long nvec = (total - head) >> 2;
  return {total, head, nvec, head + (nvec << 2), reinterpret_cast<const int4*>(id + head)};
}

// One round's vectors of thread t, four -1 where a vector lies past the last whole one.  Returns the first pixel of v[0]; v[u]'s
// is 4 * u * THREADS further on (not used as an index by a lane whose vector lies past nvec: its ids are -1, and such a pixel is
// skipped before any map is read).
__device__ __forceinline__ long long load_round(const Walk& w, int round, int t, int4 (&v)[UNROLL]) {
  const long long at0 = (long long)blockIdx.x * VECS + (long long)round * UNROLL * THREADS + t;
#pragma unroll
  for (int u = 0; u < UNROLL; ++u) {
    const long long at = at0 + (long long)u * THREADS;
    v[u] = make_int4(-1, -1, -1, -1);
    if (at < w.nvec) v[u] = w.vec[at];                    // head + 4 at + 3 < tail0 <= total
  }
  return w.head + (at0 << 2);
}

// The scalar head and tail belong to the first wave of workgroup 0, which calls pixel(e, id) as a whole: lanes 0..3 own the
// head (t < head <= total), lanes 4..7 the tail (tail0 + (t - 4) < total); a lane that owns no pixel passes (0, -1).
template <class Pixel>
__device__ __forceinline__ void scan_edges(const Walk& w, const int32_t* id, int t, Pixel&& pixel) {
  if (blockIdx.x != 0 || t >= 64) return;
  long long e = -1;
  if (t < 4) e = t < w.head ? (long long)t : -1;
  else if (t < 8) e = w.tail0 + (t - 4) < w.total ? w.tail0 + (t - 4) : -1;
  pixel(e < 0 ? 0 : e, e < 0 ? -1 : id[e]);
}

// The shared part of the rule for pixel e < total with id = pred_id[e]: its query (-1: the pixel is skipped), the stage it reached
// and its raw sensor value.  mask[e] is read only for a query with a label test, sensor[e] only for a pixel that passed it.
struct Gate { int q, stage, raw; };
__device__ __forceinline__ Gate gate(const Maps& m, size_t e, int id) {
  Gate g = {-1, OFF_MASK, 0};
  if (id < 0 || id >= m.n_meshes) return g;
  const int q = m.mesh_query[id];
  if (q < 0 || q >= m.Q) return g;
  g.q = q;
  const int label = (m.mask && m.labels) ? m.labels[q] : -2;
  if (label != -2 && !(label == -1 ? m.mask[e] != 0 : (int)m.mask[e] == label)) return g;
  g.raw = (int)m.sensor[e];
  g.stage = (g.raw == 0 || g.raw < m.raw_lo || g.raw > m.raw_hi) ? NO_MEASUREMENT : MEASURED;
  return g;
}

// The slot of query q in this workgroup's LDS (query[i] holds q + 1 of slot i's query, 0 while it is free), claiming a free
// one first come, first served; -1 when all are taken by others.
template <int SLOTS>
__device__ __forceinline__ int find_slot(int (&query)[SLOTS], int q) {
#pragma unroll
  for (int i = 0; i < SLOTS; ++i) {
    int v = *(volatile int*)&query[i];
    if (v == 0) { const int old = atomicCAS(&query[i], 0, q + 1); v = old == 0 ? q + 1 : old; }
    if (v == q + 1) return i;
  }
  return -1;
}

// One pixel per lane, pixel_q its query; the WHOLE wave calls this (lanes without a pixel pass -1).  Neighbouring pixels mostly
// belong to one query, so the wave's 64 pixels are grouped by query with ballots: body(leader, q, mine, group) runs once per query
// among them, wave-uniformly (leader: the group's first lane; group: the ballot of mine), and a group's counts are popcounts.
template <class Body>
__device__ __forceinline__ void for_each_query(int pixel_q, Body&& body) {
  unsigned long long todo = __ballot(pixel_q >= 0);
  while (todo) {
    const int leader = __ffsll((long long)todo) - 1;
    const int q = __shfl(pixel_q, leader);
    const bool mine = pixel_q == q;
    const unsigned long long group = __ballot(mine);
    todo &= ~group;
    body(leader, q, mine, group);
  }
}

// The scan grid for `total` pixels: total >> 2 is an upper bound of the whole vectors.
inline unsigned scan_blocks(long long total) { return (total >> 2) > 0 ? (unsigned)(((total >> 2) + VECS - 1) / VECS) : 1u; }

// The checks both entry points (`name`) make of the maps' arguments, in the one order their callers see, and m.total.  An entry
// point's own complaints are ranked among them and come as the text behind "name: ", or null: before_raw and after_raw about its
// scalars, buffers about its own pointers and workspace -- not looked at with Q == 0: HM_OK, no launch, nothing else is read.
inline int host_checks(const char* name, Maps& m, int N, int H, int W, const char* before_raw, const char* after_raw,
                       const char* buffers) {
  char msg[192];
  auto fail = [&](const char* text) { snprintf(msg, sizeof(msg), "%s: %s", name, text); return hm_set_error(HM_ERR_ARG, msg); };
  if (N < 1 || H < 1 || W < 1) return fail("N, H and W must be positive");
  if ((long long)N * H * W >= (1ll << 31)) return fail("N * H * W must be below 2^31");
  if (m.Q < 0 || m.n_meshes < 0) return fail("Q and n_meshes must not be negative");
  if (before_raw) return fail(before_raw);
  if (m.raw_lo > m.raw_hi) return fail("raw_lo must not exceed raw_hi");
  if (after_raw) return fail(after_raw);
  if (!m.depth || !m.id || !m.sensor) return fail("null pred_depth, pred_id or sensor");
  m.total = (long long)N * H * W;
  if (m.Q == 0) return HM_OK;
  if (buffers) return fail(buffers);
  if (((uintptr_t)m.depth & 3) || ((uintptr_t)m.id & 3) || ((uintptr_t)m.sensor & 1) || ((uintptr_t)m.labels & 3) || ((uintptr_t)m.mesh_query & 3))
    return fail("pred_depth, pred_id, labels and mesh_query must be 4-byte aligned, sensor 2-byte");
  return HM_OK;
}

}  // namespace depth_scan
