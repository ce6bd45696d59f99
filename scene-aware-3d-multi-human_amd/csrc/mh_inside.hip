// Exact points-inside-mesh query and the person-to-person penetration map (mh_mesh_bins / mh_mesh_winding / mh_person_inside,
// include/mhmocap_hip.h): is a point inside a closed triangle mesh, and how far is the surface above and below it along z.
// Read-only and off the cycle, like the contact maps in mh_contact.hip and mh_proximity.hip.
//
// Everything after the conversion of a coordinate to the lattice (X = rint(x 2^16), int32) is integer arithmetic, so the
// result is exact, the same on every launch, and equal bit for bit to an int64 brute force on the host (tests/inside_ref.py).
// The test is a ray cast along +z made robust by a symbolic perturbation of the query in x and y (the header has the rule):
// a ray through a shared edge or a vertex is counted for exactly one of the faces around it.
//
// Search structure: ONE 2D GRID PER BODY over the x and y of its lattice box.  A ray along z meets a face only if the query's
// (x, y) lies in the face's xy box, so a face is listed in every cell its closed xy box overlaps and a query looks at the ONE
// cell it falls in.  The cell edge is a power of two (a cell index is a shift): the smallest at which the grid has at most
// MI_MAX_DIM cells per axis and at most max(F / 4, MI_MIN_CELLS) cells in all -- about four faces per cell of a fine mesh, so
// that a face of such a mesh overlaps a handful of cells.  The lists of a body hold at most MI_CAP_PER_FACE F entries; a body
// that needs more (a coarse mesh of a dozen huge faces, each over most of the grid) is marked and its queries walk all F
// faces.  The result is a function of the face SET (a sum and two minima), so it is the same either way and in any order.
// The workspace keeps the lattice vertices PER FACE (three int4, 48 bytes): a face visit is three consecutive 16-byte loads,
// not an index triple followed by three gathers, and the workspace's size depends on B and F alone.
//
// Bounds, for a testable body (every finite coordinate |x| < 8192 m, lattice box at most 2^19 on every axis): |X| < 2^29;
// a query that is tested lies in the closed box, so every difference of two coordinates is at most 2^19 in magnitude and
// fits an int32; an edge function is a difference of two products of such differences, |E| <= 2^39; A = w0 + w1 + w2 is
// twice the signed area of the projected face, |A| <= 2^38; Nn is three products of a w and a z difference,
// |Nn| <= 3 2^58 < 2^61; on a covering face the w have one sign, so |Nn| <= |A| 2^19 and dz = |Nn| / |A| <= 2^19.
#include "mh_cells_p.h"
#include "mh_common.h"

#include <limits.h>
#include <math.h>

#define MI_BLOCK 256
#define MI_MAX_DIM 64
#define MI_MAX_CELLS (MI_MAX_DIM * MI_MAX_DIM)
#define MI_MIN_CELLS 256
#define MI_CAP_PER_FACE 8           // entries of a body's cell lists per face; beyond it the body walks all faces
#define MI_MAX_N 32
#define MI_MAX_EXT (1 << 19)        // lattice units: 8 m
#define MI_RANGE 8192.0f            // metres
#define MI_SCALE 65536.0f
#define MI_MAX_ITEMS (0x7fffffffll - MI_BLOCK)

#define MI_NOT_LIVE 1
#define MI_NOT_TESTABLE 2
#define MI_ALL_FACES 4

static int g_force_all_faces = 0;

struct MiHdr {                      // device-resident, one per body (written by k_mi_setup, total by k_mi_faces, flags by k_mi_scan)
  int mn[3], mx[3];                 // the lattice box of the body's finite vertices
  int shift;                        // cell edge = 2^shift lattice units
  int dx, dy;                       // cells per axis
  int flags;                        // the status word
  unsigned long long total;         // entries the cell lists would need
};

struct MiWs {                       // the layout of mh_cells_p.h
  MiHdr* hdr;                       // [B]
  int* start;                       // [B][MI_MAX_CELLS + 1]
  int* cursor;                      // [B][MI_MAX_CELLS]
  int4* rec;                        // [B][F][3]   (X, Y, Z, valid) of the three corners; valid in the first only
  int* list;                        // [B][MI_CAP_PER_FACE F]   faces by cell
};
static size_t mi_bytes(size_t B, size_t F) { return cells_bytes(B, sizeof(MiHdr), MI_MAX_CELLS, B * F * 48, B * F * MI_CAP_PER_FACE * 4); }
static MiWs mi_carve(void* ws, size_t B, size_t F) {
  const CellsWs c = cells_carve(ws, B, sizeof(MiHdr), MI_MAX_CELLS, B * F * 48);
  return {(MiHdr*)c.hdr, c.start, c.cursor, (int4*)c.a, (int*)c.b};
}

__device__ __forceinline__ bool mi_finite(float x) { return fabsf(x) < INFINITY; }            // (false for NaN)
__device__ __forceinline__ bool mi_in_range(float x) { return fabsf(x) < MI_RANGE; }          // (false for NaN and inf)
// exact scaling by a power of two, then round half to even (v_rndne_f32); |x| < 8192 keeps it inside +-2^29
__device__ __forceinline__ int mi_lattice(float x) { return (int)rintf(x * MI_SCALE); }

// ---- build: boxes, face records and totals, counts, scan, fill ----------------------------------------------------------------
// one workgroup per body: is it testable, the lattice box of its finite vertices, the grid's shape, and the cleared counts
__global__ __launch_bounds__(MI_BLOCK) void k_mi_setup(int V, int F, const float* verts, const uint8_t* live, MiHdr* hdrs, int* start) {
  __shared__ int scnt[MI_BLOCK / 64], sbad[MI_BLOCK / 64];
  __shared__ int s_nc;
  const size_t b = blockIdx.x;
  const int tid = threadIdx.x;
  const float* bv = verts + b * V * 3;
  const bool alive = !live || live[b];
  int mn[3] = {INT_MAX, INT_MAX, INT_MAX}, mx[3] = {INT_MIN, INT_MIN, INT_MIN};
  int cnt = 0, bad = 0;
  if (alive)
    for (int v = tid; v < V; v += MI_BLOCK) {
      const float p[3] = {bv[(size_t)v * 3], bv[(size_t)v * 3 + 1], bv[(size_t)v * 3 + 2]};
      bool fin = true, rng = true;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        fin = fin && mi_finite(p[c]);
        if (mi_finite(p[c]) && !mi_in_range(p[c])) { bad = 1; rng = false; }     // a finite coordinate at or beyond 8192 m
      }
      if (!fin) continue;                                  // neither in a face nor widening the box
      ++cnt;
      if (!rng) continue;                                  // (the body is not testable: its box means nothing)
#pragma unroll
      for (int c = 0; c < 3; ++c) { const int X = mi_lattice(p[c]); mn[c] = min(mn[c], X); mx[c] = max(mx[c], X); }
    }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    cnt += __shfl_xor(cnt, o, 64);
    bad |= __shfl_xor(bad, o, 64);
  }
  if ((tid & 63) == 0) { scnt[tid >> 6] = cnt; sbad[tid >> 6] = bad; }
  cells_box_reduce<MI_BLOCK>(mn, mx);                       // (its barrier publishes scnt and sbad too)
  if (tid == 0) {
    for (int w = 1; w < MI_BLOCK / 64; ++w) { cnt += scnt[w]; bad |= sbad[w]; }
    MiHdr h;
    int flags = alive ? 0 : MI_NOT_LIVE;
    if (alive && (cnt == 0 || bad)) flags |= MI_NOT_TESTABLE;
    if (flags == 0)                                        // (|X| < 2^29: the differences fit)
      for (int c = 0; c < 3; ++c)
        if (mx[c] - mn[c] > MI_MAX_EXT) flags |= MI_NOT_TESTABLE;
    int shift = 0, dx = 1, dy = 1;
    if (flags == 0) {
      const int ex = mx[0] - mn[0], ey = mx[1] - mn[1];
      const int most = max(F / 4, MI_MIN_CELLS);
      for (;; ++shift) {                                   // ends at shift = 19 at the latest: one cell
        dx = (ex >> shift) + 1; dy = (ey >> shift) + 1;
        if (dx <= MI_MAX_DIM && dy <= MI_MAX_DIM && dx * dy <= most) break;
      }
    } else {
      for (int c = 0; c < 3; ++c) { mn[c] = 0; mx[c] = -1; }                   // an empty box: no query is in it
    }
    for (int c = 0; c < 3; ++c) { h.mn[c] = mn[c]; h.mx[c] = mx[c]; }
    h.shift = shift; h.dx = dx; h.dy = dy; h.flags = flags; h.total = 0ull;
    hdrs[b] = h;
    s_nc = flags == 0 ? dx * dy : 0;
  }
  __syncthreads();
  const int nc = s_nc;
  int* counts = start + b * (MI_MAX_CELLS + 1);
  for (int i = tid; i <= nc; i += MI_BLOCK) counts[i] = 0;
}

__device__ __forceinline__ bool mi_walks_all(const MiHdr& h, int F, int force) { return force != 0 || cells_over_cap(h.total, F, MI_CAP_PER_FACE); }

struct MiGrid {                     // the face grid of mh_cells_p.h: two-dimensional, over x and y of the lattice
  typedef MiHdr Hdr;
  typedef int4 Rec;
  static constexpr int BLOCK = MI_BLOCK, MAX_CELLS = MI_MAX_CELLS, CAP_PER_FACE = MI_CAP_PER_FACE;
  static __device__ __forceinline__ bool counted(const MiHdr& h, int F, int force) {
    return !(h.flags & (MI_NOT_LIVE | MI_NOT_TESTABLE)) && !mi_walks_all(h, F, force);
  }
  static __device__ __forceinline__ bool valid(const int4& r) { return r.w != 0; }
  // the cells [c0, c1] of x and y that the closed xy box of a face record overlaps (one layer: z is not binned)
  static __device__ __forceinline__ void range(const MiHdr& h, const int4 a, const int4 b, const int4 c, int c0[3], int c1[3]) {
    c0[0] = (min(a.x, min(b.x, c.x)) - h.mn[0]) >> h.shift;
    c1[0] = (max(a.x, max(b.x, c.x)) - h.mn[0]) >> h.shift;
    c0[1] = (min(a.y, min(b.y, c.y)) - h.mn[1]) >> h.shift;
    c1[1] = (max(a.y, max(b.y, c.y)) - h.mn[1]) >> h.shift;
    c0[0] = max(c0[0], 0); c0[1] = max(c0[1], 0);          // (a finite vertex of a testable body is inside its box: never clips)
    c1[0] = min(c1[0], h.dx - 1); c1[1] = min(c1[1], h.dy - 1);
    c0[2] = c1[2] = 0;
  }
  static __device__ __forceinline__ int cell(const MiHdr& h, int cx, int cy, int) { return cy * h.dx + cx; }
};

// one lane per (body, face), the workgroups of a body consecutive: the face's lattice record, and the entries it would need
__global__ __launch_bounds__(MI_BLOCK) void k_mi_faces(int V, int F, int fpb, const float* verts, const int* faces, MiHdr* hdrs, int4* rec) {
  __shared__ int s_total;
  const int tid = threadIdx.x;
  size_t b;
  const int f = cells_body_face<MI_BLOCK>(fpb, b);
  if (tid == 0) s_total = 0;
  __syncthreads();
  const MiHdr h = hdrs[b];
  if (f < F) {
    int4 r[3] = {make_int4(0, 0, 0, 0), make_int4(0, 0, 0, 0), make_int4(0, 0, 0, 0)};
    const int i[3] = {faces[(size_t)f * 3], faces[(size_t)f * 3 + 1], faces[(size_t)f * 3 + 2]};
    bool ok = (h.flags & (MI_NOT_LIVE | MI_NOT_TESTABLE)) == 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) ok = ok && i[k] >= 0 && i[k] < V;
    if (ok) {
      const float* bv = verts + b * V * 3;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const float x = bv[(size_t)i[k] * 3], y = bv[(size_t)i[k] * 3 + 1], z = bv[(size_t)i[k] * 3 + 2];
        // (testable: a finite coordinate is in range; the test of the range keeps the conversion defined whatever comes)
        if (mi_in_range(x) && mi_in_range(y) && mi_in_range(z)) r[k] = make_int4(mi_lattice(x), mi_lattice(y), mi_lattice(z), 0);
        else ok = false;
      }
    }
    r[0].w = ok ? 1 : 0;
    int4* o = rec + (b * F + f) * 3;
    o[0] = r[0]; o[1] = r[1]; o[2] = r[2];
    if (ok) {
      int c0[3], c1[3];
      MiGrid::range(h, r[0], r[1], r[2], c0, c1);
      atomicAdd(&s_total, (c1[0] - c0[0] + 1) * (c1[1] - c0[1] + 1));          // (<= 256 x 4096: no overflow)
    }
  }
  __syncthreads();
  if (tid == 0 && s_total != 0) atomicAdd(&hdrs[b].total, (unsigned long long)s_total);
}

// (the counts and the fill are k_cells_count<MiGrid> and k_cells_fill<MiGrid>: at most 8 F atomics a body)

// one workgroup per body: the path it takes and its status word; exclusive scan of its counts in place, and the fill cursors
__global__ __launch_bounds__(1024) void k_mi_scan(int F, int force, MiHdr* hdrs, int* start, int* cursor, int* status) {
  const size_t b = blockIdx.x;
  const MiHdr h = hdrs[b];
  const bool testable = (h.flags & (MI_NOT_LIVE | MI_NOT_TESTABLE)) == 0;
  const bool all = testable && mi_walks_all(h, F, force);
  if (threadIdx.x == 0) {
    const int flags = h.flags | (all ? MI_ALL_FACES : 0);
    hdrs[b].flags = flags;
    if (status) status[b] = flags;
  }
  if (!testable || all) return;                            // (uniform over the workgroup)
  cells_scan_1024(min(h.dx * h.dy, MI_MAX_CELLS), start + b * (MI_MAX_CELLS + 1), cursor + b * MI_MAX_CELLS);
}

// ---- the test of one face ---------------------------------------------------------------------------------------------------------
// the sign of the directed edge a -> b at the query under the perturbation Q + (eps, eps^2), and the edge function itself
__device__ __forceinline__ int mi_edge(int xa, int ya, int xb, int yb, int qx, int qy, long long& E) {
  const int dx = xb - xa, dy = yb - ya;
  E = (long long)dx * (qy - ya) - (long long)dy * (qx - xa);
  if (E != 0) return E > 0 ? 1 : -1;
  if (dy != 0) return dy > 0 ? -1 : 1;
  return (dx > 0) - (dx < 0);
}

struct MiAcc {
  int winding;
  unsigned up, down;               // ~0u: none (which reads -1 as an int32)
};

__device__ __forceinline__ void mi_face(const int4* __restrict__ r, int qx, int qy, int qz, MiAcc& acc) {
  const int4 p0 = r[0], p1 = r[1], p2 = r[2];
  if (!p0.w) return;
  long long w0, w1, w2;
  const int s0 = mi_edge(p1.x, p1.y, p2.x, p2.y, qx, qy, w0);
  const int s1 = mi_edge(p2.x, p2.y, p0.x, p0.y, qx, qy, w1);
  const int s2 = mi_edge(p0.x, p0.y, p1.x, p1.y, qx, qy, w2);
  const long long A = w0 + w1 + w2;
  if (A == 0 || s0 == 0 || s0 != s1 || s1 != s2) return;   // does not cover the query
  const long long Nn = w0 * (long long)(p0.z - qz) + w1 * (long long)(p1.z - qz) + w2 * (long long)(p2.z - qz);
  if (Nn == 0) return;                                     // the query is on the face: neither above nor below
  const unsigned long long an = Nn < 0 ? 0ull - (unsigned long long)Nn : (unsigned long long)Nn;
  const unsigned long long aa = A < 0 ? 0ull - (unsigned long long)A : (unsigned long long)A;
  const unsigned dz = (unsigned)(an / aa);
  if ((Nn > 0) == (A > 0)) {
    acc.winding += A > 0 ? 1 : -1;
    acc.up = min(acc.up, dz);
  } else {
    acc.down = min(acc.down, dz);
  }
}

// the query (qx, qy, qz) against one testable body; false: outside its closed lattice box
__device__ __forceinline__ bool mi_query(const MiHdr& h, int F, const int4* __restrict__ rec, const int* __restrict__ start,
                                         const int* __restrict__ list, int qx, int qy, int qz, MiAcc& acc) {
  if (qx < h.mn[0] || qx > h.mx[0] || qy < h.mn[1] || qy > h.mx[1] || qz < h.mn[2] || qz > h.mx[2]) return false;
  if (h.flags & MI_ALL_FACES) {
    for (int f = 0; f < F; ++f) mi_face(rec + (size_t)f * 3, qx, qy, qz, acc);
  } else {
    const int c = ((qy - h.mn[1]) >> h.shift) * h.dx + ((qx - h.mn[0]) >> h.shift);
    cells_visit(start, list, c, F, MI_CAP_PER_FACE, [&](int f) { mi_face(rec + (size_t)f * 3, qx, qy, qz, acc); });
  }
  return true;
}

// a float query on the lattice; false: not finite, or so far out that it is outside every testable body's box
__device__ __forceinline__ bool mi_query_lattice(const float* p, int& qx, int& qy, int& qz) {
  const float x = p[0], y = p[1], z = p[2];
  if (!(mi_in_range(x) && mi_in_range(y) && mi_in_range(z))) return false;
  qx = mi_lattice(x); qy = mi_lattice(y); qz = mi_lattice(z);
  return true;
}

// ---- the generic query: points b against body b, one lane per point ----------------------------------------------------------
struct WindingP {
  int total, Q, F;
  const float* points;
  const MiHdr* hdr;
  const int* start;
  const int* list;
  const int4* rec;
  int* winding;
  int* up;
  int* down;
};

__global__ __launch_bounds__(MI_BLOCK) void k_mesh_winding(WindingP p) {
  const int i = blockIdx.x * MI_BLOCK + threadIdx.x;
  if (i >= p.total) return;
  const size_t b = (size_t)(i / p.Q);
  MiAcc acc = {0, ~0u, ~0u};
  const MiHdr h = p.hdr[b];
  int qx, qy, qz;
  if (!(h.flags & (MI_NOT_LIVE | MI_NOT_TESTABLE)) && mi_query_lattice(p.points + (size_t)i * 3, qx, qy, qz))
    mi_query(h, p.F, p.rec + b * p.F * 3, p.start + b * (MI_MAX_CELLS + 1), p.list + b * (size_t)p.F * MI_CAP_PER_FACE, qx, qy, qz, acc);
  if (p.winding) p.winding[i] = acc.winding;
  if (p.up) p.up[i] = (int)acc.up;
  if (p.down) p.down[i] = (int)acc.down;
}

// ---- the penetration map: one lane per vertex, walking the other bodies of its frame ----------------------------------------
struct InsideP {
  int N, V, F, P, bpb;              // workgroups per body
  const float* verts;
  const uint8_t* part;
  const MiHdr* hdr;
  const int* start;
  const int* list;
  const int4* rec;
  unsigned* mask;
  int* depth;
  int* other;
  int* pair_verts;
  int* pair_depth;
  int* part_verts;
  int* part_depth;
};

__global__ __launch_bounds__(MI_BLOCK) void k_person_inside(InsideP p) {
  __shared__ int s_pv[MI_MAX_N], s_pd[MI_MAX_N], s_cv[MI_MAX_N], s_cd[MI_MAX_N];
  const int tid = threadIdx.x;
  const int b = blockIdx.x / p.bpb, v = (blockIdx.x - b * p.bpb) * MI_BLOCK + tid;         // b = t N + n
  const int N = p.N, V = p.V, F = p.F;
  const int t = b / N, n = b - t * N;
  if (tid < MI_MAX_N) { s_pv[tid] = 0; s_pd[tid] = -1; s_cv[tid] = 0; s_cd[tid] = -1; }
  __syncthreads();
  if (v < V) {
    const size_t i = (size_t)b * V + v;
    unsigned mask = 0;
    int depth = -1, other = -1;
    int qx, qy, qz;
    if (!(p.hdr[b].flags & MI_NOT_LIVE) && mi_query_lattice(p.verts + i * 3, qx, qy, qz)) {
      for (int m = 0; m < N; ++m) {
        if (m == n) continue;                              // its own body: never a container
        const size_t bm = (size_t)t * N + m;
        const MiHdr h = p.hdr[bm];
        if (h.flags & (MI_NOT_LIVE | MI_NOT_TESTABLE)) continue;
        MiAcc acc = {0, ~0u, ~0u};
        if (!mi_query(h, F, p.rec + bm * F * 3, p.start + bm * (MI_MAX_CELLS + 1), p.list + bm * (size_t)F * MI_CAP_PER_FACE, qx, qy, qz, acc))
          continue;                                        // the box misses the query
        if (acc.winding == 0) continue;
        const int ex = (int)min(acc.up, acc.down);         // (inside: a face above exists, so up does)
        mask |= 1u << m;
        if (ex > depth) { depth = ex; other = m; }         // ascending m: the smallest m on a tie
        atomicAdd(&s_pv[m], 1);
        atomicMax(&s_pd[m], ex);
      }
      if (mask) {
        const int k = p.part[v];
        if (k < p.P) { atomicAdd(&s_cv[k], 1); atomicMax(&s_cd[k], depth); }
      }
    }
    if (p.mask) p.mask[i] = mask;
    if (p.depth) p.depth[i] = depth;
    if (p.other) p.other[i] = other;
  }
  __syncthreads();
  if (tid < N) {
    const size_t o = (size_t)b * N + tid;
    if (p.pair_verts && s_pv[tid] != 0) atomicAdd(&p.pair_verts[o], s_pv[tid]);
    if (p.pair_depth && s_pd[tid] >= 0) atomicMax(&p.pair_depth[o], s_pd[tid]);
  }
  if (tid < p.P) {
    const size_t o = (size_t)b * p.P + tid;
    if (p.part_verts && s_cv[tid] != 0) atomicAdd(&p.part_verts[o], s_cv[tid]);
    if (p.part_depth && s_cd[tid] >= 0) atomicMax(&p.part_depth[o], s_cd[tid]);
  }
}

// ---- entry points ------------------------------------------------------------------------------------------------------------------
extern "C" int mh_mesh_set_all_faces(int on) {
  const int was = g_force_all_faces;
  g_force_all_faces = on ? 1 : 0;
  return was;
}

extern "C" size_t mh_mesh_bins_bytes(int B, int F) { return mi_bytes((size_t)(B > 0 ? B : 1), (size_t)(F > 0 ? F : 1)); }

extern "C" int mh_mesh_bins(int B, int V, int F, const float* verts, const int32_t* faces, const uint8_t* live, void* ws, size_t ws_bytes,
                            int32_t* status, void* stream) {
  MH_CHECK(B > 0 && V > 0 && F > 0, "empty input");
  MH_CHECK((long long)B * V <= MI_MAX_ITEMS, "too many vertices for one launch (B * V): call it on fewer bodies");
  MH_CHECK((long long)B * F <= MI_MAX_ITEMS / MI_CAP_PER_FACE, "too many faces for one launch (8 B * F must stay below 2^31): call it on fewer bodies");
  MH_CHECK(verts && faces && ws, "null argument: verts, faces and ws");
  MH_CHECK(ws_bytes >= mh_mesh_bins_bytes(B, F), "workspace too small: ws_bytes is below mh_mesh_bins_bytes(B, F)");
  const int fpb = (F + MI_BLOCK - 1) / MI_BLOCK;
  const unsigned nblk = (unsigned)((size_t)B * fpb);
  const int force = g_force_all_faces;
  MiWs w = mi_carve(ws, (size_t)B, (size_t)F);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_mi_setup, dim3((unsigned)B), dim3(MI_BLOCK), 0, st, V, F, verts, live, w.hdr, w.start);
  MH_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_mi_faces, dim3(nblk), dim3(MI_BLOCK), 0, st, V, F, fpb, verts, faces, w.hdr, w.rec);
  MH_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_cells_count<MiGrid>, dim3(nblk), dim3(MI_BLOCK), 0, st, F, fpb, force, (const MiHdr*)w.hdr, (const int4*)w.rec, w.start);
  MH_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_mi_scan, dim3((unsigned)B), dim3(1024), 0, st, F, force, w.hdr, w.start, w.cursor, status);
  MH_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_cells_fill<MiGrid>, dim3(nblk), dim3(MI_BLOCK), 0, st, F, fpb, (const MiHdr*)w.hdr, (const int4*)w.rec, w.cursor, w.list);
  MH_LAUNCH_CHECK();
  return MH_OK;
}

extern "C" int mh_mesh_winding(int B, int V, int F, const int32_t* faces, const void* ws, int Q, const float* points, int32_t* winding,
                               int32_t* up, int32_t* down, void* stream) {
  MH_CHECK(B > 0 && V > 0 && F > 0 && Q > 0, "empty input");
  MH_CHECK((long long)B * Q <= MI_MAX_ITEMS, "too many points for one launch (B * Q): call it on fewer points");
  MH_CHECK((long long)B * F <= MI_MAX_ITEMS / MI_CAP_PER_FACE, "too many faces for one launch (8 B * F must stay below 2^31): call it on fewer bodies");
  MH_CHECK(faces && ws && points, "null argument: faces, ws and points");
  MH_CHECK(winding || up || down, "no output requested (every output is null)");
  MiWs w = mi_carve((void*)ws, (size_t)B, (size_t)F);
  WindingP p;
  p.total = B * Q; p.Q = Q; p.F = F;
  p.points = points;
  p.hdr = w.hdr; p.start = w.start; p.list = w.list; p.rec = w.rec;
  p.winding = winding; p.up = up; p.down = down;
  hipLaunchKernelGGL(k_mesh_winding, dim3((unsigned)((p.total + MI_BLOCK - 1) / MI_BLOCK)), dim3(MI_BLOCK), 0, (hipStream_t)stream, p);
  MH_LAUNCH_CHECK();
  return MH_OK;
}

extern "C" int mh_person_inside(int T, int N, int V, int F, const int32_t* faces, const void* ws, const float* verts, const uint8_t* part, int P,
                                uint32_t* mask, int32_t* depth, int32_t* other, int32_t* pair_verts, int32_t* pair_depth,
                                int32_t* part_verts, int32_t* part_depth, void* stream) {
  MH_CHECK(T > 0 && N > 0 && V > 0 && F > 0, "empty input");
  MH_CHECK(N <= MI_MAX_N, "N must be at most 32 people per frame");
  MH_CHECK(P >= 1 && P <= MI_MAX_N, "P must be in 1..32");
  MH_CHECK((long long)T * N * V <= MI_MAX_ITEMS, "too many vertices for one launch (T * N * V): call it on fewer frames");
  MH_CHECK((long long)T * N * F <= MI_MAX_ITEMS / MI_CAP_PER_FACE, "too many faces for one launch (8 T * N * F must stay below 2^31): call it on fewer frames");
  MH_CHECK(faces && ws && verts && part, "null argument: faces, ws, verts and part");
  MH_CHECK(mask || depth || other || pair_verts || pair_depth || part_verts || part_depth, "no output requested (every output is null)");
  const size_t B = (size_t)T * N;
  MiWs w = mi_carve((void*)ws, B, (size_t)F);
  InsideP p;
  p.N = N; p.V = V; p.F = F; p.P = P;
  p.bpb = (V + MI_BLOCK - 1) / MI_BLOCK;
  p.verts = verts; p.part = part;
  p.hdr = w.hdr; p.start = w.start; p.list = w.list; p.rec = w.rec;
  p.mask = mask; p.depth = depth; p.other = other;
  p.pair_verts = pair_verts; p.pair_depth = pair_depth; p.part_verts = part_verts; p.part_depth = part_depth;
  hipStream_t st = (hipStream_t)stream;
  if (pair_verts) MH_HIP(hipMemsetAsync(pair_verts, 0, B * N * sizeof(int32_t), st));
  if (pair_depth) MH_HIP(hipMemsetAsync(pair_depth, 0xff, B * N * sizeof(int32_t), st));
  if (part_verts) MH_HIP(hipMemsetAsync(part_verts, 0, B * P * sizeof(int32_t), st));
  if (part_depth) MH_HIP(hipMemsetAsync(part_depth, 0xff, B * P * sizeof(int32_t), st));
  hipLaunchKernelGGL(k_person_inside, dim3((unsigned)(B * p.bpb)), dim3(MI_BLOCK), 0, st, p);
  MH_LAUNCH_CHECK();
  return MH_OK;
}
