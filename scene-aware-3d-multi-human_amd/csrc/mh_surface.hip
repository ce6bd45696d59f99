// Exact point-to-surface distance and the person-to-person clearance map (mh_surface_grid / mh_mesh_closest / mh_person_surface /
// mh_surface_pairs, include/mhmocap_hip.h): for a point the nearest point of a triangle mesh, and for every vertex of every
// person the nearest surface among the other people of its frame and, where mh_person_inside says it is inside somebody, how
// far it is from that body's surface -- the shortest way out.  Read-only and off the cycle, like the maps in mh_proximity.hip
// and mh_inside.hip.
//
// The arithmetic of a face visit is written in the order the header states and compiled without contraction: a float32
// evaluation of the same expressions on the host gives the same bits (tests/surface_ref.py).  The result is a function of the
// candidate SET (smallest D2, then smallest face), so the search structure decides the cost and nothing else.
//
// Search structure: ONE 3D UNIFORM GRID OF FACE LISTS PER BODY over the box of its finite vertices, cubic cells of edge h.
//   cell_a(x) = clamp(floor((x - mn_a) * inv), 0, d_a - 1),  inv = 1 / h  (float32; a NaN goes to 0)
// is MONOTONE in x on every axis.  A face with box [lo, hi] is listed in every cell of cell(lo) .. cell(hi).  h is the smallest
// of the sequence maxext / 64 * 1.0625^i at which the grid has at most MS_MAX_DIM cells per axis and at most
// min(max(F / 2, MS_MIN_CELLS), MS_MAX_CELLS) cells in all (for the body model: 14 x 54 x 9 cells of 3.1 cm, 1.4 mean edges).  The
// lists of a body hold at most MS_CAP_PER_FACE F entries; a body that needs more (a coarse mesh of a dozen huge faces), or
// whose box overflows float32, is marked and its queries walk all F faces.  The workspace keeps the corners PER FACE (three
// float4, 48 bytes), as mh_inside.hip does: a face visit is three 16-byte loads.
//
// The query walks RINGS of cells around cq = cell(q) (the cell of the query clamped into the box), ring k = the cells at
// Chebyshev index distance k, nearest first, and stops when a lower bound on the distance to everything not yet visited
// exceeds the best D2 (or r2).  Every trip count comes from the grid: at most max(d_a) rings, each cell visited once, so a
// query 1000 m away with an unbounded radius costs one pass over the body's cells.
//
// WHY THE PRUNING LOSES NO CANDIDATE.  After ring k every cell within index distance k of cq has been visited.  A face f that
// was not visited has a cell range disjoint from that cube of cells, so on some axis a its range lies wholly above cq_a + k or
// wholly below cq_a - k.  Above: cell_a(lo_a) >= j = cq_a + k + 1, that is fl(fl(lo_a - mn_a) inv) >= j, and with
// inv = (1 + e) / h, two more roundings, lo_a - mn_a >= j h (1 - 3 eps) (eps = 2^-24): EVERY point p of the face has
// p_a - q_a >= (mn_a + j h) - q_a - 3 eps j h.  Below: cell_a(hi_a) <= cq_a - k - 1 (this index is below d_a - 1, so the clamp did
// not produce it), hi_a - mn_a < (cq_a - k) h (1 + 3 eps), and q_a - p_a >= q_a - (mn_a + (cq_a - k) h) - 3 eps (cq_a - k) h.  The
// kernel's bound g is the smallest of these gaps over the axes and directions in which unvisited cells exist, evaluated in
// float32 (three roundings, each at most eps times max(|mn_a|, |mx_a|, |q_a|) + h) and then LOWERED to g (1 - 2^-10) - slack,
// slack = 2^-16 (S + max|q_a|), S = max_a max(|mn_a|, |mx_a|) + h: 2^-16 S is over a thousand times the roundings just named.
// The other side of the comparison is the COMPUTED D2 of the unvisited face, which may lie below its true squared distance
// dist(q, f)^2: the corner differences A, B, C, ab, ac carry a relative error eps each, the computed closest point
// x = A + ab v + ac w an absolute error of a few eps (|A| + |ab| + |ac|) <= a few eps (dist + 2 diam(f)) <= 2^-20 (S + |q|), and
// v, w themselves lie in the triangle up to rounding (the vertex and edge regions give them from quotients in [0, 1] by
// construction; the interior region from vb / den, vc / den, whose error moves x inside the face's plane by a few eps diam(f)
// for a face that is not a sliver beyond float32's reach) -- all of it inside the slack with a factor of ten to spare, and
// dot(x, x) adds 3 eps relative, far inside 2^-10.  So an unvisited face has computed D2 > (g lowered)^2 whenever that is
// positive, and the walk stops only when (g lowered)^2 is STRICTLY greater than min(best D2, r2): a face that ties the best D2
// with a smaller index is never pruned.  The same bound with the box itself (k = "before the first ring") drops a whole body.
// INSIDE A RING the same bound is taken per layer, row and cell: the closest point p* of a face lies in the face's box, on
// every axis in one of the slabs cell_a(lo_a) .. cell_a(hi_a) (consecutive slabs overlap by their rounding margins and cover
// [lo_a, hi_a]), so it lies in a cell c* that lists the face, and |p* - q|^2 >= the sum over the axes of the squared gaps
// between q and c*'s slabs.  Each gap is lowered as above before it is squared (lowering every component of a non-negative
// vector by s lowers its norm by at least s), so a cell is skipped only when no face whose closest point lies in it can be a
// candidate or tie the best; a face skipped there is met through c* or is none.  Without this a ring of 26 cells was walked
// whole although the best face so far was nearer than most of them.
// The test of the claim is tests/test_surface_gpu.py: the grid path and the forced all-faces path must agree bit for bit.
#include "mh_cells_p.h"
#include "mh_common.h"

#include <float.h>
#include <math.h>

#pragma clang fp contract(off)

#define MS_BLOCK 256
#define MS_MAX_DIM 64
#define MS_MAX_CELLS 8192
#define MS_MIN_CELLS 256
#define MS_CAP_PER_FACE 16          // entries of a body's cell lists per face; beyond it the body walks all faces
#define MS_SHAPE_STEPS 128          // 1.0625^128 > 2000: from 64 cells on the longest axis to one cell and beyond
#define MS_MAX_N 32
#define MS_INF_BITS 0x7f800000u
#define MS_NONE_BITS 0xbf800000u    // -1.0f: below the bits of every non-negative float as an int32
#define MS_MAX_ITEMS (0x7fffffffll - MS_BLOCK)
#define MS_REL 0.9990234375f        // 1 - 2^-10
#define MS_SLACK 1.52587890625e-05f // 2^-16

#define MS_NOT_LIVE 1
#define MS_ALL_FACES 4

static int g_surface_all_faces = 0;

struct MsHdr {                      // device-resident, one per body (written by k_ms_setup, total by k_ms_faces, flags by k_ms_scan)
  float mn[3], mx[3];               // the box of the body's finite vertices, exact
  float h, inv;                     // cell edge and 1 / h
  float scale;                      // S of the slack: max_a max(|mn_a|, |mx_a|) + h
  int d[3];                         // cells per axis
  int flags;                        // the status word
  int overflow;                     // the box's extent is not finite: no grid
  unsigned long long total;         // entries the cell lists would need
};

struct MsWs {                       // the layout of mh_cells_p.h
  MsHdr* hdr;                       // [B]
  int* start;                       // [B][MS_MAX_CELLS + 1]
  int* cursor;                      // [B][MS_MAX_CELLS]
  float4* rec;                      // [B][F][3]   (x, y, z, valid) of the three corners; valid in the first only
  int* list;                        // [B][MS_CAP_PER_FACE F]   faces by cell
};
static size_t ms_bytes(size_t B, size_t F) { return cells_bytes(B, sizeof(MsHdr), MS_MAX_CELLS, B * F * 48, B * F * MS_CAP_PER_FACE * 4); }
static MsWs ms_carve(void* ws, size_t B, size_t F) {
  const CellsWs c = cells_carve(ws, B, sizeof(MsHdr), MS_MAX_CELLS, B * F * 48);
  return {(MsHdr*)c.hdr, c.start, c.cursor, (float4*)c.a, (int*)c.b};
}

__device__ __forceinline__ bool ms_finite(float x) { return fabsf(x) < INFINITY; }            // (false for NaN)

// the cell of a coordinate on one axis: monotone in x; the clamps are taken on the float, so a NaN product goes to cell 0
__device__ __forceinline__ int ms_cell(float x, float mn, float inv, int d) {
  return (int)fminf(fmaxf(floorf((x - mn) * inv), 0.f), (float)(d - 1));
}

__device__ __forceinline__ bool ms_sane(const MsHdr& h) {                                    // a header that k_ms_setup wrote
  return h.d[0] >= 1 && h.d[1] >= 1 && h.d[2] >= 1 && h.d[0] <= MS_MAX_DIM && h.d[1] <= MS_MAX_DIM && h.d[2] <= MS_MAX_DIM &&
         h.d[0] * h.d[1] * h.d[2] <= MS_MAX_CELLS;
}

// ---- build: boxes, face records and totals, counts, scan, fill ----------------------------------------------------------------
// one workgroup per body: the box of its finite vertices, the grid's shape, and the cleared counts
__global__ __launch_bounds__(MS_BLOCK) void k_ms_setup(int V, int F, const float* verts, const uint8_t* live, MsHdr* hdrs, int* start) {
  __shared__ int s_nc;
  const size_t b = blockIdx.x;
  const int tid = threadIdx.x;
  const float* bv = verts + b * V * 3;
  const bool alive = !live || live[b];
  float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
  if (alive)
    for (int v = tid; v < V; v += MS_BLOCK) {
      const float p[3] = {bv[(size_t)v * 3], bv[(size_t)v * 3 + 1], bv[(size_t)v * 3 + 2]};
      if (!(ms_finite(p[0]) && ms_finite(p[1]) && ms_finite(p[2]))) continue;   // neither in a face nor widening the box
#pragma unroll
      for (int c = 0; c < 3; ++c) { mn[c] = fminf(mn[c], p[c]); mx[c] = fmaxf(mx[c], p[c]); }
    }
  cells_box_reduce<MS_BLOCK>(mn, mx);
  if (tid == 0) {
    MsHdr h;
    h.flags = alive ? 0 : MS_NOT_LIVE;
    h.overflow = 0;
    h.total = 0ull;
    h.d[0] = h.d[1] = h.d[2] = 1;
    h.h = 1.f;
    if (!(mn[0] <= mx[0])) {                               // dead, or no finite vertex: no face is listed, nothing is found
      for (int c = 0; c < 3; ++c) { mn[c] = 0.f; mx[c] = 0.f; }
    } else {
      const float ext[3] = {mx[0] - mn[0], mx[1] - mn[1], mx[2] - mn[2]};
      const float maxext = fmaxf(ext[0], fmaxf(ext[1], ext[2]));
      if (!ms_finite(maxext)) {
        h.overflow = 1;
      } else if (maxext >= 1e-30f) {                       // (below it: one cell; 1 / h stays finite above it)
        const int most = min(max(F / 2, MS_MIN_CELLS), MS_MAX_CELLS);
        float e = maxext / (float)MS_MAX_DIM;
        bool fits = false;
        for (int it = 0; it < MS_SHAPE_STEPS && !fits; ++it) {
          for (int c = 0; c < 3; ++c) h.d[c] = (int)fminf(floorf(ext[c] / e), (float)(MS_MAX_DIM - 1)) + 1;
          fits = h.d[0] * h.d[1] * h.d[2] <= most;
          if (!fits) e = e * 1.0625f;
        }
        if (fits) h.h = e;
        else h.d[0] = h.d[1] = h.d[2] = 1;                 // (not reached: most >= 256 admits 6 cells per axis)
      }
    }
    h.inv = 1.f / h.h;
    float s = 0.f;
    for (int c = 0; c < 3; ++c) { h.mn[c] = mn[c]; h.mx[c] = mx[c]; s = fmaxf(s, fmaxf(fabsf(mn[c]), fabsf(mx[c]))); }
    h.scale = s + h.h;
    hdrs[b] = h;
    s_nc = h.d[0] * h.d[1] * h.d[2];
  }
  __syncthreads();
  const int nc = s_nc;
  int* counts = start + b * (MS_MAX_CELLS + 1);
  for (int i = tid; i <= nc; i += MS_BLOCK) counts[i] = 0;
}

__device__ __forceinline__ bool ms_walks_all(const MsHdr& h, int F, int force) {
  return force != 0 || h.overflow != 0 || cells_over_cap(h.total, F, MS_CAP_PER_FACE);
}

struct MsGrid {                     // the face grid of mh_cells_p.h: three-dimensional
  typedef MsHdr Hdr;
  typedef float4 Rec;
  static constexpr int BLOCK = MS_BLOCK, MAX_CELLS = MS_MAX_CELLS, CAP_PER_FACE = MS_CAP_PER_FACE;
  static __device__ __forceinline__ bool counted(const MsHdr& h, int F, int force) { return !(h.flags & MS_NOT_LIVE) && !ms_walks_all(h, F, force); }
  static __device__ __forceinline__ bool valid(const float4& r) { return r.w != 0.f; }
  // the cells [c0, c1] per axis that the box of a face record overlaps
  static __device__ __forceinline__ void range(const MsHdr& h, const float4 a, const float4 b, const float4 c, int c0[3], int c1[3]) {
    const float lo[3] = {fminf(a.x, fminf(b.x, c.x)), fminf(a.y, fminf(b.y, c.y)), fminf(a.z, fminf(b.z, c.z))};
    const float hi[3] = {fmaxf(a.x, fmaxf(b.x, c.x)), fmaxf(a.y, fmaxf(b.y, c.y)), fmaxf(a.z, fmaxf(b.z, c.z))};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      c0[k] = ms_cell(lo[k], h.mn[k], h.inv, h.d[k]);
      c1[k] = max(ms_cell(hi[k], h.mn[k], h.inv, h.d[k]), c0[k]);
    }
  }
  static __device__ __forceinline__ int cell(const MsHdr& h, int cx, int cy, int cz) { return (cz * h.d[1] + cy) * h.d[0] + cx; }
};

// one lane per (body, face), the workgroups of a body consecutive: the face's record, and the entries it would need
__global__ __launch_bounds__(MS_BLOCK) void k_ms_faces(int V, int F, int fpb, const float* verts, const int* faces, MsHdr* hdrs, float4* rec) {
  __shared__ int s_total;
  const int tid = threadIdx.x;
  size_t b;
  const int f = cells_body_face<MS_BLOCK>(fpb, b);
  if (tid == 0) s_total = 0;
  __syncthreads();
  const MsHdr h = hdrs[b];
  if (f < F) {
    float4 r[3] = {make_float4(0.f, 0.f, 0.f, 0.f), make_float4(0.f, 0.f, 0.f, 0.f), make_float4(0.f, 0.f, 0.f, 0.f)};
    const int i[3] = {faces[(size_t)f * 3], faces[(size_t)f * 3 + 1], faces[(size_t)f * 3 + 2]};
    bool ok = (h.flags & MS_NOT_LIVE) == 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) ok = ok && i[k] >= 0 && i[k] < V;
    if (ok) {
      const float* bv = verts + b * V * 3;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const float x = bv[(size_t)i[k] * 3], y = bv[(size_t)i[k] * 3 + 1], z = bv[(size_t)i[k] * 3 + 2];
        if (ms_finite(x) && ms_finite(y) && ms_finite(z)) r[k] = make_float4(x, y, z, 0.f);
        else ok = false;
      }
    }
    r[0].w = ok ? 1.f : 0.f;
    float4* o = rec + (b * F + f) * 3;
    o[0] = r[0]; o[1] = r[1]; o[2] = r[2];
    if (ok && !h.overflow) {
      int c0[3], c1[3];
      MsGrid::range(h, r[0], r[1], r[2], c0, c1);
      atomicAdd(&s_total, (c1[0] - c0[0] + 1) * (c1[1] - c0[1] + 1) * (c1[2] - c0[2] + 1));      // (<= 256 x 8192: no overflow)
    }
  }
  __syncthreads();
  if (tid == 0 && s_total != 0) atomicAdd(&hdrs[b].total, (unsigned long long)s_total);
}

// (the counts and the fill are k_cells_count<MsGrid> and k_cells_fill<MsGrid>: at most 16 F atomics a body)

// one workgroup per body: the path it takes and its status word; exclusive scan of its counts in place, and the fill cursors
__global__ __launch_bounds__(1024) void k_ms_scan(int F, int force, MsHdr* hdrs, int* start, int* cursor, int* status) {
  const size_t b = blockIdx.x;
  const MsHdr h = hdrs[b];
  const bool alive = (h.flags & MS_NOT_LIVE) == 0;
  const bool all = alive && ms_walks_all(h, F, force);
  if (threadIdx.x == 0) {
    const int flags = h.flags | (all ? MS_ALL_FACES : 0);
    hdrs[b].flags = flags;
    if (status) status[b] = flags;
  }
  if (!alive || all) return;                               // (uniform over the workgroup)
  cells_scan_1024(min(h.d[0] * h.d[1] * h.d[2], MS_MAX_CELLS), start + b * (MS_MAX_CELLS + 1), cursor + b * MS_MAX_CELLS);
}

// ---- the visit of one face: the header's formula, in its order ------------------------------------------------------------------
struct MsBest {
  float d2;                         // +inf: none yet
  int f;                            // -1: none yet (as unsigned, above every face index: a first candidate with D2 = +inf wins)
  float x[3];                       // closest point - query
  float v, w;
};

__device__ __forceinline__ float ms_dot(const float u[3], const float v[3]) { return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]; }

__device__ __forceinline__ void ms_face(const float4* __restrict__ r, int f, const float q[3], float r2, MsBest& best, int& visits) {
  const float4 p0 = r[0], p1 = r[1], p2 = r[2];
  if (p0.w == 0.f) return;
  ++visits;
  const float A[3] = {p0.x - q[0], p0.y - q[1], p0.z - q[2]};
  const float B[3] = {p1.x - q[0], p1.y - q[1], p1.z - q[2]};
  const float C[3] = {p2.x - q[0], p2.y - q[1], p2.z - q[2]};
  const float ab[3] = {p1.x - p0.x, p1.y - p0.y, p1.z - p0.z};
  const float ac[3] = {p2.x - p0.x, p2.y - p0.y, p2.z - p0.z};
  const float d1 = -ms_dot(ab, A), d2 = -ms_dot(ac, A), d3 = -ms_dot(ab, B), d4 = -ms_dot(ac, B), d5 = -ms_dot(ab, C), d6 = -ms_dot(ac, C);
  const float vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4, e1 = d4 - d3, e2 = d5 - d6;
  float v, w;
  if (d1 <= 0.f && d2 <= 0.f) { v = 0.f; w = 0.f; }
  else if (d3 >= 0.f && d4 <= d3) { v = 1.f; w = 0.f; }
  else if (vc <= 0.f && d1 >= 0.f && d3 <= 0.f) { v = d1 / (d1 - d3); w = 0.f; }
  else if (d6 >= 0.f && d5 <= d6) { v = 0.f; w = 1.f; }
  else if (vb <= 0.f && d2 >= 0.f && d6 <= 0.f) { v = 0.f; w = d2 / (d2 - d6); }
  else if (va <= 0.f && e1 >= 0.f && e2 >= 0.f) { const float t = e1 / (e1 + e2); v = 1.f - t; w = t; }
  else { const float den = (va + vb) + vc; v = vb / den; w = vc / den; }
  const float x[3] = {(A[0] + ab[0] * v) + ac[0] * w, (A[1] + ab[1] * v) + ac[1] * w, (A[2] + ab[2] * v) + ac[2] * w};
  const float D2 = ms_dot(x, x);
  if (!(D2 <= r2)) return;                                 // beyond the radius, or NaN: no candidate
  if (D2 < best.d2 || (D2 == best.d2 && (unsigned)f < (unsigned)best.f)) {
    best.d2 = D2; best.f = f;
    best.x[0] = x[0]; best.x[1] = x[1]; best.x[2] = x[2];
    best.v = v; best.w = w;
  }
}

// lowers a gap to what the header comment argues is a bound on the computed D2 of everything beyond it; true: nothing beyond
// the gap can be a candidate or beat (or tie) the best
__device__ __forceinline__ bool ms_beyond(float gap, float slack, float limit) {
  const float g = gap * MS_REL - slack;
  return g > 0.f && g * g > limit;
}

// how far the query is, on one axis, from the slab of the cells with index j on that axis, lowered in the same way; 0 inside
// the slab.  The points p with cell_a(p) = j have mn_a + j h (1 - 3 eps) <= p_a < mn_a + (j + 1) h (1 + 3 eps); in the first and
// last slab the box itself is the bound (the clamp sends everything beyond to them).  A bound that overflowed prunes nothing.
__device__ __forceinline__ float ms_slab_gap(const MsHdr& h, int a, int j, float q, float slack) {
  const float lo = j == 0 ? h.mn[a] : h.mn[a] + (float)j * h.h;
  const float hi = j == h.d[a] - 1 ? h.mx[a] : h.mn[a] + (float)(j + 1) * h.h;
  const float g = fmaxf(lo - q, q - hi) * MS_REL - slack;
  return g > 0.f && g < INFINITY ? g : 0.f;
}

// the query against one live body: false iff the body was dropped at its box (grown by the radius)
__device__ __forceinline__ bool ms_search(const MsHdr& h, int F, const float4* __restrict__ rec, const int* __restrict__ start,
                                          const int* __restrict__ list, const float q[3], float r2, bool box_test, MsBest& best, int& visits) {
  const float slack = (h.scale + fmaxf(fabsf(q[0]), fmaxf(fabsf(q[1]), fabsf(q[2])))) * MS_SLACK;
  if (box_test && r2 < INFINITY) {
#pragma unroll
    for (int a = 0; a < 3; ++a)
      if (ms_beyond(h.mn[a] - q[a], slack, r2) || ms_beyond(q[a] - h.mx[a], slack, r2)) return false;
  }
  if ((h.flags & MS_ALL_FACES) || !ms_sane(h)) {
    if (h.flags & MS_ALL_FACES)
      for (int f = 0; f < F; ++f) ms_face(rec + (size_t)f * 3, f, q, r2, best, visits);
    return true;
  }
  int cq[3], K = 0;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    cq[a] = ms_cell(q[a], h.mn[a], h.inv, h.d[a]);
    K = max(K, max(cq[a], h.d[a] - 1 - cq[a]));
  }
  for (int k = 0; k <= K; ++k) {                           // K < MS_MAX_DIM rings, every cell of the grid at most once
    const int z0 = max(cq[2] - k, 0), z1 = min(cq[2] + k, h.d[2] - 1);
    const int y0 = max(cq[1] - k, 0), y1 = min(cq[1] + k, h.d[1] - 1);
    const int x0 = max(cq[0] - k, 0), x1 = min(cq[0] + k, h.d[0] - 1);
    for (int cz = z0; cz <= z1; ++cz) {
      const float gz = ms_slab_gap(h, 2, cz, q[2], slack);
      if (gz * gz > fminf(best.d2, r2)) continue;           // the whole layer of cells is too far
      for (int cy = y0; cy <= y1; ++cy) {
        const float gy = ms_slab_gap(h, 1, cy, q[1], slack);
        const float gzy = gz * gz + gy * gy;
        if (gzy > fminf(best.d2, r2)) continue;             // the whole row
        const bool shell = abs(cz - cq[2]) == k || abs(cy - cq[1]) == k;
        // a row of the ring's shell is walked whole; of an inner row only the two end cells belong to ring k
        const int step = shell ? 1 : max(2 * k, 1);
        for (int cx = cq[0] - k; cx <= cq[0] + k; cx += step) {
          if (cx < x0 || cx > x1) continue;
          const float gx = ms_slab_gap(h, 0, cx, q[0], slack);
          if (gzy + gx * gx > fminf(best.d2, r2)) continue; // the cell
          const int c = (cz * h.d[1] + cy) * h.d[0] + cx;
          cells_visit(start, list, c, F, MS_CAP_PER_FACE, [&](int f) { ms_face(rec + (size_t)f * 3, f, q, r2, best, visits); });
        }
      }
    }
    float gap = INFINITY;                                 // over the axes and directions in which cells remain
    bool remain = false;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      if (cq[a] + k + 1 <= h.d[a] - 1) { remain = true; gap = fminf(gap, (h.mn[a] + (float)(cq[a] + k + 1) * h.h) - q[a]); }
      if (cq[a] - k - 1 >= 0) { remain = true; gap = fminf(gap, q[a] - (h.mn[a] + (float)(cq[a] - k) * h.h)); }
    }
    if (!remain) break;                                    // every cell has been visited
    if (gap < INFINITY && ms_beyond(gap, slack, fminf(best.d2, r2))) break;      // (an overflowed bound prunes nothing)
  }
  return true;
}

__device__ __forceinline__ bool ms_finite3(const float q[3]) { return ms_finite(q[0]) && ms_finite(q[1]) && ms_finite(q[2]); }

// ---- the generic query: points b against body b, one lane per point ----------------------------------------------------------
struct ClosestP {
  int total, Q, F;
  float r2;
  const float* points;
  const MsHdr* hdr;
  const int* start;
  const int* list;
  const float4* rec;
  float* d2;
  int* face;
  float* point;
  float* weights;
};

__global__ __launch_bounds__(MS_BLOCK) void k_mesh_closest(ClosestP p) {
  const int i = blockIdx.x * MS_BLOCK + threadIdx.x;
  if (i >= p.total) return;
  const size_t b = (size_t)(i / p.Q);
  MsBest best = {INFINITY, -1, {0.f, 0.f, 0.f}, 0.f, 0.f};
  const MsHdr h = p.hdr[b];
  const float q[3] = {p.points[(size_t)i * 3], p.points[(size_t)i * 3 + 1], p.points[(size_t)i * 3 + 2]};
  int visits = 0;
  if (!(h.flags & MS_NOT_LIVE) && ms_finite3(q))
    ms_search(h, p.F, p.rec + b * p.F * 3, p.start + b * (MS_MAX_CELLS + 1), p.list + b * (size_t)p.F * MS_CAP_PER_FACE, q, p.r2, true, best,
              visits);
  const bool found = best.f >= 0;
  if (p.d2) p.d2[i] = best.d2;
  if (p.face) p.face[i] = best.f;
  if (p.point)
    for (int c = 0; c < 3; ++c) p.point[(size_t)i * 3 + c] = found ? q[c] + best.x[c] : 0.f;
  if (p.weights) {
    p.weights[(size_t)i * 3] = found ? (1.f - best.v) - best.w : 0.f;
    p.weights[(size_t)i * 3 + 1] = found ? best.v : 0.f;
    p.weights[(size_t)i * 3 + 2] = found ? best.w : 0.f;
  }
}

// ---- the clearance map: one lane per vertex, walking the other bodies of its frame ------------------------------------------
struct SurfaceP {
  int N, V, F, bpb;                 // workgroups per body
  float r2;
  const float* verts;
  const unsigned* mask;
  const MsHdr* hdr;
  const int* start;
  const int* list;
  const float4* rec;
  float* out_d2;
  int* out_idx;
  float* in_d2;
  int* in_idx;
  float* out_pt;
  float* in_pt;
  int* stats;
};

__global__ __launch_bounds__(MS_BLOCK) void k_person_surface(SurfaceP p) {
  const int b = blockIdx.x / p.bpb, v = (blockIdx.x - b * p.bpb) * MS_BLOCK + threadIdx.x;       // b = t N + n
  const int N = p.N, V = p.V, F = p.F;
  if (v >= V) return;
  const int t = b / N, n = b - t * N;
  const size_t i = (size_t)b * V + v;
  float od = INFINITY, id = -1.f;
  int oi = -1, ii = -1;
  float ox[3] = {0.f, 0.f, 0.f}, ix[3] = {0.f, 0.f, 0.f};
  int bodies = 0, visits = 0;
  const float q[3] = {p.verts[i * 3], p.verts[i * 3 + 1], p.verts[i * 3 + 2]};
  if (!(p.hdr[b].flags & MS_NOT_LIVE) && ms_finite3(q)) {
    const unsigned mask = p.mask ? p.mask[i] : 0u;
    for (int m = 0; m < N; ++m) {
      if (m == n) continue;
      const size_t bm = (size_t)t * N + m;
      const MsHdr h = p.hdr[bm];
      if (h.flags & MS_NOT_LIVE) continue;
      const bool inside = (mask >> m) & 1u;
      MsBest best = {INFINITY, -1, {0.f, 0.f, 0.f}, 0.f, 0.f};
      // inside m: unbounded, and no box test -- the vertex is in m's box, the walk ends after a few rings
      if (!ms_search(h, F, p.rec + bm * F * 3, p.start + bm * (MS_MAX_CELLS + 1), p.list + bm * (size_t)F * MS_CAP_PER_FACE, q,
                     inside ? INFINITY : p.r2, !inside, best, visits))
        continue;
      ++bodies;
      if (best.f < 0) continue;
      if (inside) {
        if (best.d2 > id) {                                // ascending m: the smallest m on a tie
          id = best.d2; ii = m * F + best.f;
          ix[0] = best.x[0]; ix[1] = best.x[1]; ix[2] = best.x[2];
        }
      } else if (oi < 0 || best.d2 < od) {
        od = best.d2; oi = m * F + best.f;
        ox[0] = best.x[0]; ox[1] = best.x[1]; ox[2] = best.x[2];
      }
    }
  }
  if (p.out_d2) p.out_d2[i] = od;
  if (p.out_idx) p.out_idx[i] = oi;
  if (p.in_d2) p.in_d2[i] = ii >= 0 ? id : INFINITY;
  if (p.in_idx) p.in_idx[i] = ii;
  if (p.out_pt)
    for (int c = 0; c < 3; ++c) p.out_pt[i * 3 + c] = oi >= 0 ? q[c] + ox[c] : 0.f;
  if (p.in_pt)
    for (int c = 0; c < 3; ++c) p.in_pt[i * 3 + c] = ii >= 0 ? q[c] + ix[c] : 0.f;
  if (p.stats) { p.stats[i * 2] = bodies; p.stats[i * 2 + 1] = visits; }
}

// ---- the per-pair and per-part tables ---------------------------------------------------------------------------------------------
struct SPairsP {
  int N, V, F, P, bpb;
  float c2;
  const float* out_d2;
  const int* out_idx;
  const float* in_d2;
  const int* in_idx;
  const uint8_t* part;
  int* pair_depth;                  // float bits as int32: the values compared are >= 0, whose bits order like their values
  unsigned* pair_min;
  int* pair_contact;
  int* part_depth;
  unsigned* part_min;
  int* part_contact;
};

__global__ __launch_bounds__(MS_BLOCK) void k_surface_pairs(SPairsP p) {
  __shared__ int s_pd[MS_MAX_N], s_pc[MS_MAX_N], s_cd[MS_MAX_N], s_cc[MS_MAX_N];
  __shared__ unsigned s_pm[MS_MAX_N], s_cm[MS_MAX_N];
  const int tid = threadIdx.x;
  const int b = blockIdx.x / p.bpb, v = (blockIdx.x - b * p.bpb) * MS_BLOCK + tid;               // b = t N + n
  const int N = p.N, V = p.V, F = p.F;
  if (tid < MS_MAX_N) {
    s_pd[tid] = (int)MS_NONE_BITS; s_cd[tid] = (int)MS_NONE_BITS; s_pc[tid] = 0; s_cc[tid] = 0;
    s_pm[tid] = MS_INF_BITS; s_cm[tid] = MS_INF_BITS;
  }
  __syncthreads();
  if (v < V) {
    const size_t i = (size_t)b * V + v;
    const int k = p.part[v];
    const int oi = p.out_idx[i], ii = p.in_idx[i];
    if (oi >= 0 && oi / F < N) {                           // (an index beyond the frame's bodies is followed nowhere)
      const int m = oi / F;
      const float d = p.out_d2[i];
      const bool touch = d <= p.c2;
      if (touch) atomicAdd(&s_pc[m], 1);
      if (touch && k < p.P) atomicAdd(&s_cc[k], 1);
      if (d >= 0.f) {                                      // NaN and negative values are never a minimum
        const unsigned bits = __float_as_uint(d + 0.f);    // (-0 + 0 = +0)
        atomicMin(&s_pm[m], bits);
        if (k < p.P) atomicMin(&s_cm[k], bits);
      }
    }
    if (ii >= 0 && ii / F < N) {
      const int m = ii / F;
      const float d = p.in_d2[i];
      if (d >= 0.f) {
        const int bits = (int)__float_as_uint(d + 0.f);
        atomicMax(&s_pd[m], bits);
        if (k < p.P) atomicMax(&s_cd[k], bits);
      }
    }
  }
  __syncthreads();
  if (tid < N) {
    const size_t o = (size_t)b * N + tid;
    if (p.pair_depth && s_pd[tid] >= 0) atomicMax(&p.pair_depth[o], s_pd[tid]);
    if (p.pair_min && s_pm[tid] != MS_INF_BITS) atomicMin(&p.pair_min[o], s_pm[tid]);
    if (p.pair_contact && s_pc[tid] != 0) atomicAdd(&p.pair_contact[o], s_pc[tid]);
  }
  if (tid < p.P) {
    const size_t o = (size_t)b * p.P + tid;
    if (p.part_depth && s_cd[tid] >= 0) atomicMax(&p.part_depth[o], s_cd[tid]);
    if (p.part_min && s_cm[tid] != MS_INF_BITS) atomicMin(&p.part_min[o], s_cm[tid]);
    if (p.part_contact && s_cc[tid] != 0) atomicAdd(&p.part_contact[o], s_cc[tid]);
  }
}

// ---- entry points ------------------------------------------------------------------------------------------------------------------
extern "C" int mh_surface_set_all_faces(int on) {
  const int was = g_surface_all_faces;
  g_surface_all_faces = on ? 1 : 0;
  return was;
}

extern "C" size_t mh_surface_grid_bytes(int B, int F) { return ms_bytes((size_t)(B > 0 ? B : 1), (size_t)(F > 0 ? F : 1)); }

extern "C" int mh_surface_grid(int B, int V, int F, const float* verts, const int32_t* faces, const uint8_t* live, void* ws, size_t ws_bytes,
                               int32_t* status, void* stream) {
  MH_CHECK(B > 0 && V > 0 && F > 0, "empty input");
  MH_CHECK((long long)B * V <= MS_MAX_ITEMS, "too many vertices for one launch (B * V): call it on fewer bodies");
  MH_CHECK((long long)B * F <= MS_MAX_ITEMS / MS_CAP_PER_FACE, "too many faces for one launch (16 B * F must stay below 2^31): call it on fewer bodies");
  MH_CHECK(verts && faces && ws, "null argument: verts, faces and ws");
  MH_CHECK(ws_bytes >= mh_surface_grid_bytes(B, F), "workspace too small: ws_bytes is below mh_surface_grid_bytes(B, F)");
  const int fpb = (F + MS_BLOCK - 1) / MS_BLOCK;
  const unsigned nblk = (unsigned)((size_t)B * fpb);
  const int force = g_surface_all_faces;
  MsWs w = ms_carve(ws, (size_t)B, (size_t)F);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_ms_setup, dim3((unsigned)B), dim3(MS_BLOCK), 0, st, V, F, verts, live, w.hdr, w.start);
  MH_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_ms_faces, dim3(nblk), dim3(MS_BLOCK), 0, st, V, F, fpb, verts, faces, w.hdr, w.rec);
  MH_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_cells_count<MsGrid>, dim3(nblk), dim3(MS_BLOCK), 0, st, F, fpb, force, (const MsHdr*)w.hdr, (const float4*)w.rec, w.start);
  MH_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_ms_scan, dim3((unsigned)B), dim3(1024), 0, st, F, force, w.hdr, w.start, w.cursor, status);
  MH_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_cells_fill<MsGrid>, dim3(nblk), dim3(MS_BLOCK), 0, st, F, fpb, (const MsHdr*)w.hdr, (const float4*)w.rec, w.cursor, w.list);
  MH_LAUNCH_CHECK();
  return MH_OK;
}

extern "C" int mh_mesh_closest(int B, int V, int F, const int32_t* faces, const void* ws, int Q, const float* points, float radius, float* d2,
                               int32_t* face, float* point, float* weights, void* stream) {
  MH_CHECK(B > 0 && V > 0 && F > 0 && Q > 0, "empty input");
  MH_CHECK((long long)B * Q <= MS_MAX_ITEMS, "too many points for one launch (B * Q): call it on fewer points");
  MH_CHECK((long long)B * F <= MS_MAX_ITEMS / MS_CAP_PER_FACE, "too many faces for one launch (16 B * F must stay below 2^31): call it on fewer bodies");
  MH_CHECK(faces && ws && points, "null argument: faces, ws and points");
  MH_CHECK(d2 || face || point || weights, "no output requested (every output is null)");
  MH_CHECK(radius > 0.f, "radius must be positive (+inf is allowed)");
  MsWs w = ms_carve((void*)ws, (size_t)B, (size_t)F);
  ClosestP p;
  p.total = B * Q; p.Q = Q; p.F = F;
  p.r2 = radius * radius;
  p.points = points;
  p.hdr = w.hdr; p.start = w.start; p.list = w.list; p.rec = w.rec;
  p.d2 = d2; p.face = face; p.point = point; p.weights = weights;
  hipLaunchKernelGGL(k_mesh_closest, dim3((unsigned)((p.total + MS_BLOCK - 1) / MS_BLOCK)), dim3(MS_BLOCK), 0, (hipStream_t)stream, p);
  MH_LAUNCH_CHECK();
  return MH_OK;
}

extern "C" int mh_person_surface(int T, int N, int V, int F, const int32_t* faces, const void* ws, const float* verts, const uint32_t* mask,
                                 float radius, float* out_d2, int32_t* out_idx, float* in_d2, int32_t* in_idx, float* out_pt, float* in_pt,
                                 int32_t* stats, void* stream) {
  MH_CHECK(T > 0 && N > 0 && V > 0 && F > 0, "empty input");
  MH_CHECK(N <= MS_MAX_N, "N must be at most 32 people per frame");
  MH_CHECK((long long)N * F <= 0x7fffffffll, "N * F must stay below 2^31: idx = m * F + f is an int32");
  MH_CHECK((long long)T * N * V <= MS_MAX_ITEMS, "too many vertices for one launch (T * N * V): call it on fewer frames");
  MH_CHECK((long long)T * N * F <= MS_MAX_ITEMS / MS_CAP_PER_FACE,
           "too many faces for one launch (16 T * N * F must stay below 2^31): call it on fewer frames");
  MH_CHECK(faces && ws && verts, "null argument: faces, ws and verts");
  MH_CHECK(out_d2 || out_idx || in_d2 || in_idx || out_pt || in_pt || stats, "no output requested (every output is null)");
  MH_CHECK(radius > 0.f, "radius must be positive (+inf is allowed)");
  const size_t B = (size_t)T * N;
  MsWs w = ms_carve((void*)ws, B, (size_t)F);
  SurfaceP p;
  p.N = N; p.V = V; p.F = F;
  p.bpb = (V + MS_BLOCK - 1) / MS_BLOCK;
  p.r2 = radius * radius;
  p.verts = verts; p.mask = mask;
  p.hdr = w.hdr; p.start = w.start; p.list = w.list; p.rec = w.rec;
  p.out_d2 = out_d2; p.out_idx = out_idx; p.in_d2 = in_d2; p.in_idx = in_idx; p.out_pt = out_pt; p.in_pt = in_pt; p.stats = stats;
  hipLaunchKernelGGL(k_person_surface, dim3((unsigned)(B * p.bpb)), dim3(MS_BLOCK), 0, (hipStream_t)stream, p);
  MH_LAUNCH_CHECK();
  return MH_OK;
}

extern "C" int mh_surface_pairs(int T, int N, int V, int F, const float* out_d2, const int32_t* out_idx, const float* in_d2,
                                const int32_t* in_idx, const uint8_t* part, int P, float contact, float* pair_depth_d2, float* pair_min_d2,
                                int32_t* pair_contact, float* part_depth_d2, float* part_min_d2, int32_t* part_contact, void* stream) {
  MH_CHECK(T > 0 && N > 0 && V > 0 && F > 0, "empty input");
  MH_CHECK(N <= MS_MAX_N, "N must be at most 32 people per frame");
  MH_CHECK(P >= 1 && P <= MS_MAX_N, "P must be in 1..32");
  MH_CHECK((long long)N * F <= 0x7fffffffll, "N * F must stay below 2^31: idx = m * F + f is an int32");
  MH_CHECK((long long)T * N * V <= MS_MAX_ITEMS, "too many vertices for one launch (T * N * V): call it on fewer frames");
  MH_CHECK(out_d2 && out_idx && in_d2 && in_idx && part, "null argument: out_d2, out_idx, in_d2, in_idx and part");
  MH_CHECK(pair_depth_d2 || pair_min_d2 || pair_contact || part_depth_d2 || part_min_d2 || part_contact,
           "no output requested (every output is null)");
  MH_CHECK(contact >= 0.f && contact < INFINITY, "contact must be finite and not negative");
  SPairsP p;
  p.N = N; p.V = V; p.F = F; p.P = P;
  p.bpb = (V + MS_BLOCK - 1) / MS_BLOCK;
  p.c2 = contact * contact;
  p.out_d2 = out_d2; p.out_idx = out_idx; p.in_d2 = in_d2; p.in_idx = in_idx; p.part = part;
  p.pair_depth = (int*)pair_depth_d2; p.pair_min = (unsigned*)pair_min_d2; p.pair_contact = pair_contact;
  p.part_depth = (int*)part_depth_d2; p.part_min = (unsigned*)part_min_d2; p.part_contact = part_contact;
  const size_t B = (size_t)T * N;
  hipStream_t st = (hipStream_t)stream;
  if (pair_depth_d2) MH_HIP(hipMemsetD32Async((hipDeviceptr_t)pair_depth_d2, (int)MS_NONE_BITS, B * N, st));
  if (pair_min_d2) MH_HIP(hipMemsetD32Async((hipDeviceptr_t)pair_min_d2, (int)MS_INF_BITS, B * N, st));
  if (pair_contact) MH_HIP(hipMemsetAsync(pair_contact, 0, B * N * sizeof(int32_t), st));
  if (part_depth_d2) MH_HIP(hipMemsetD32Async((hipDeviceptr_t)part_depth_d2, (int)MS_NONE_BITS, B * P, st));
  if (part_min_d2) MH_HIP(hipMemsetD32Async((hipDeviceptr_t)part_min_d2, (int)MS_INF_BITS, B * P, st));
  if (part_contact) MH_HIP(hipMemsetAsync(part_contact, 0, B * P * sizeof(int32_t), st));
  hipLaunchKernelGGL(k_surface_pairs, dim3((unsigned)(B * p.bpb)), dim3(MS_BLOCK), 0, st, p);
  MH_LAUNCH_CHECK();
  return MH_OK;
}
