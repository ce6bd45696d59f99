// Person-to-person contact map (mh_vertex_normals / mh_person_nearest / mh_person_pairs, include/mhmocap_hip.h): for every
// vertex of every body the nearest vertex of the OTHER bodies of its frame within a radius, on which side of that body's
// surface it lies, and per pair of people and per body part how many vertices touch and how close they come.  Read-only and
// off the cycle, like the body-to-scene map in mh_contact.hip.
//
// Search structure: ONE SMALL UNIFORM GRID PER BODY, not per frame.  A grid over all bodies of a frame would make every
// query wade through its own body's vertices -- by far the nearest points to it -- before it met anyone else's.  With a grid
// per body a lane walks the OTHER bodies of its frame and drops a body whose bounding box, grown by the radius, misses the
// query after reading that body's header; most people in most frames do not touch, so this is where most (vertex, body)
// pairs end.  Every grid has at most PN_MAX_CELLS cells (a table of 16 KB), so a chunk of 8 frames x 32 people needs a few
// MB of tables beside the sorted vertices.  All grids of a call are built by four launches over the chunk (boxes, counts,
// scan, scatter) with integer atomics only; the order of the vertices inside a cell varies from launch to launch, the
// result does not: it is a function of the SET of candidates (smallest d2, then smallest person, then smallest vertex).
//
// The arithmetic is written in the order the header states and compiled without contraction: a float32 evaluation of the
// same expressions on the host gives the same bits (tests/proximity_ref.py).
#include "mh_cells_p.h"
#include "mh_common.h"

#include <float.h>
#include <math.h>

#pragma clang fp contract(off)

#define PN_BLOCK 256
#define PN_MAX_CELLS 4096
#define PN_MIN_CELL 0.02f
#define PN_MAX_N 32
#define PN_MAX_RADIUS 0.64          // the cap of mh_scene_nearest: MH_SCENE_NEAREST_MAX_CELLS cells of 0.02 m
#define PN_INF_BITS 0x7f800000u
#define PN_MAX_ITEMS (0x7fffffffll - PN_BLOCK)

struct PnHdr {          // device-resident, one per body (written by k_pn_setup)
  float mn[3], mx[3];   // the bounding box of the body's finite vertices, exact
  float cell;
  int dim[3];
  int ncells;
  int npts;             // finite vertices of a live body; 0: nothing to find here
};

struct PnWs {         // the layout of mh_cells_p.h
  PnHdr* hdr;        // [B]
  int* start;        // [B][PN_MAX_CELLS + 1]
  int* cursor;       // [B][PN_MAX_CELLS]
  int* pcell;        // [B][V]   cell of every vertex, -1: not binned
  uint4* sorted;     // [B][V]   (x, y, z bits, vertex index) by cell
};
static size_t pn_bytes(size_t B, size_t V) { return cells_bytes(B, sizeof(PnHdr), PN_MAX_CELLS, B * V * 4, B * V * 16); }
static PnWs pn_carve(void* ws, size_t B, size_t V) {
  const CellsWs c = cells_carve(ws, B, sizeof(PnHdr), PN_MAX_CELLS, B * V * 4);
  return {(PnHdr*)c.hdr, c.start, c.cursor, (int*)c.a, (uint4*)c.b};
}

__device__ __forceinline__ bool pn_finite3(float x, float y, float z) {
  return fabsf(x) < INFINITY && fabsf(y) < INFINITY && fabsf(z) < INFINITY;                            // (false for NaN)
}

// The cell of coordinate p on one axis.  Monotone in p: the subtraction of a constant and the division by a positive
// constant round monotonically (an overflow to +-inf included), so do the two clamps and the truncation.  mn is finite
// wherever this is called, so no NaN arises; the clamp in float keeps the conversion in range whatever p is.
__device__ __forceinline__ int pn_cell1(float p, float mn, float cell, int dim) {
  return (int)fminf(fmaxf((p - mn) / cell, 0.f), (float)(dim - 1));
}

// Cells [c0, c1] of one axis that can hold a candidate of a query at coordinate q; false: the body's box misses the query.
//
// Superset, by the argument of sn_axis (mh_contact.hip), which carries over word for word: a candidate has
// fl(fl(dx dx + dy dy) + dz dz) <= fl(r r) with dx = fl(p - q); rounding is monotone and the other squares are >= 0, so
// fl(dx dx) <= fl(r r).  With rp = max(r (1 + 2^-20), 1e-12) rounded (>= r (1 + 2^-21)), |dx| >= rp would give
// fl(dx dx) >= rp rp (1 - 2^-24) > r r (1 + 2^-24) >= fl(r r): every candidate has |fl(p - q)| < rp.
// L = the float below fl(q - rp) is <= q - rp in the reals; a float p < L has p - q < -rp, hence fl(p - q) <= -rp: not a
// candidate.  So L <= p, and likewise p <= U = the float above fl(q + rp).
// Box: mn and mx are the smallest and largest coordinate of the body's binned vertices exactly, so U < mn or L > mx leaves
// no candidate.  Cells: pn_cell1 is monotone and is the function the build bins with, so c(L) <= c(p) <= c(U).
__device__ __forceinline__ bool pn_axis(float q, float rp, float mn, float mx, float cell, int dim, int& c0, int& c1) {
  const float L = nextafterf(q - rp, -INFINITY), U = nextafterf(q + rp, INFINITY);
  if (U < mn || L > mx) return false;
  c0 = pn_cell1(L, mn, cell, dim);
  c1 = pn_cell1(U, mn, cell, dim);
  return true;
}

// ---- build: boxes, counts, scan, scatter -------------------------------------------------------------------------------------
// one workgroup per body: the box of its finite vertices, the grid's shape, and the cleared counts
__global__ __launch_bounds__(PN_BLOCK) void k_pn_setup(int V, const float* verts, const uint8_t* live, PnHdr* hdrs, int* start) {
  __shared__ int scnt[PN_BLOCK / 64];
  __shared__ int s_nc;
  const size_t b = blockIdx.x;
  const int tid = threadIdx.x;
  const float* bv = verts + b * V * 3;
  float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
  int cnt = 0;
  if (!live || live[b])
    for (int v = tid; v < V; v += PN_BLOCK) {
      const float p[3] = {bv[(size_t)v * 3], bv[(size_t)v * 3 + 1], bv[(size_t)v * 3 + 2]};
      if (!pn_finite3(p[0], p[1], p[2])) continue;        // neither binned nor widening the box
      ++cnt;
#pragma unroll
      for (int c = 0; c < 3; ++c) { mn[c] = fminf(mn[c], p[c]); mx[c] = fmaxf(mx[c], p[c]); }
    }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
  if ((tid & 63) == 0) scnt[tid >> 6] = cnt;
  cells_box_reduce<PN_BLOCK>(mn, mx);                       // (its barrier publishes scnt too)
  if (tid == 0) {
    for (int w = 1; w < PN_BLOCK / 64; ++w) cnt += scnt[w];
    PnHdr h;
    h.npts = cnt;
    float ext[3];
    bool wide = false;                                   // an extent that overflows float32
    for (int c = 0; c < 3; ++c) {
      if (cnt == 0) { mn[c] = 0.f; mx[c] = 0.f; }
      ext[c] = fmaxf(mx[c] - mn[c], 1e-3f);              // (a body of zero extent: one cell)
      wide = wide || !(ext[c] < INFINITY);
      h.mn[c] = mn[c]; h.mx[c] = mx[c];
    }
    int d[3] = {1, 1, 1};
    float cell = FLT_MAX;                                // wide: one cell that holds everything
    if (!wide) {
      // about PN_MAX_CELLS cells over the volume of the box, never below PN_MIN_CELL; grown until the table holds them
      cell = fmaxf(cbrtf(ext[0]) * cbrtf(ext[1]) * cbrtf(ext[2]) / 16.f, PN_MIN_CELL);
      for (;;) {
        int n = 1;                                       // (each factor <= PN_MAX_CELLS + 1: n stays far below 2^31 where it matters)
        bool fits = true;
        for (int c = 0; c < 3; ++c) {
          d[c] = (int)fminf(ext[c] / cell, (float)PN_MAX_CELLS) + 1;
          fits = fits && n <= PN_MAX_CELLS / d[c];
          n = fits ? n * d[c] : n;
        }
        if (fits) break;
        cell *= 1.26f;
      }
    }
    h.cell = cell;
    for (int c = 0; c < 3; ++c) h.dim[c] = d[c];
    h.ncells = d[0] * d[1] * d[2];
    hdrs[b] = h;
    s_nc = h.ncells;
  }
  __syncthreads();
  const int nc = s_nc;
  int* counts = start + b * (PN_MAX_CELLS + 1);
  for (int i = tid; i <= nc; i += PN_BLOCK) counts[i] = 0;
}

// one lane per (body, vertex): its cell, counted
__global__ __launch_bounds__(PN_BLOCK) void k_pn_count(int total, int V, const float* verts, const PnHdr* hdrs, int* start, int* pcell) {
  const int i = blockIdx.x * PN_BLOCK + threadIdx.x;
  if (i >= total) return;
  const size_t b = (size_t)(i / V);
  const PnHdr* h = hdrs + b;
  const float x = verts[(size_t)i * 3], y = verts[(size_t)i * 3 + 1], z = verts[(size_t)i * 3 + 2];
  int c = -1;
  if (h->npts > 0 && pn_finite3(x, y, z)) {
    const int cx = pn_cell1(x, h->mn[0], h->cell, h->dim[0]);
    const int cy = pn_cell1(y, h->mn[1], h->cell, h->dim[1]);
    const int cz = pn_cell1(z, h->mn[2], h->cell, h->dim[2]);
    c = (cz * h->dim[1] + cy) * h->dim[0] + cx;
    atomicAdd(&start[b * (PN_MAX_CELLS + 1) + c], 1);
  }
  pcell[i] = c;
}

// one workgroup per body: exclusive scan of its counts[0..ncells] in place, and the fill cursors
__global__ __launch_bounds__(1024) void k_pn_scan(const PnHdr* hdrs, int* start, int* cursor) {
  const size_t b = blockIdx.x;
  cells_scan_1024(min(hdrs[b].ncells, PN_MAX_CELLS), start + b * (PN_MAX_CELLS + 1), cursor + b * PN_MAX_CELLS);
}

__global__ __launch_bounds__(PN_BLOCK) void k_pn_scatter(int total, int V, const float* verts, const int* pcell, int* cursor, uint4* sorted) {
  const int i = blockIdx.x * PN_BLOCK + threadIdx.x;
  if (i >= total) return;
  const int c = pcell[i];
  if (c < 0 || c >= PN_MAX_CELLS) return;
  const size_t b = (size_t)(i / V);
  const int v = i - (int)b * V;
  const int pos = atomicAdd(&cursor[b * PN_MAX_CELLS + c], 1);
  if ((unsigned)pos >= (unsigned)V) return;            // (cannot happen after the count; a lane never leaves its body's slab)
  sorted[b * V + pos] = make_uint4(__float_as_uint(verts[(size_t)i * 3]), __float_as_uint(verts[(size_t)i * 3 + 1]),
                                   __float_as_uint(verts[(size_t)i * 3 + 2]), (unsigned)v);
}

// ---- query: one lane per vertex, walking the other bodies of its frame -----------------------------------------------------
struct PersonNearestP {
  int total, N, V;
  float radius;
  const float* verts;
  const uint8_t* live;
  const PnHdr* hdr;
  const int* start;
  const uint4* sorted;
  float* d2;
  int* idx;
};

__global__ __launch_bounds__(PN_BLOCK) void k_person_nearest(PersonNearestP p) {
  const int i = blockIdx.x * PN_BLOCK + threadIdx.x;
  if (i >= p.total) return;
  const int V = p.V, N = p.N;
  const int b = i / V, t = b / N, n = b - t * N;
  const float qx = p.verts[(size_t)i * 3], qy = p.verts[(size_t)i * 3 + 1], qz = p.verts[(size_t)i * 3 + 2];
  float bd = INFINITY;
  int bi = -1;
  if ((!p.live || p.live[b]) && pn_finite3(qx, qy, qz)) {
    const float r2 = p.radius * p.radius;
    const float rp = fmaxf(p.radius * 1.000001f, 1e-12f);
    for (int m = 0; m < N; ++m) {
      if (m == n) continue;                              // its own body: never a candidate
      const size_t bm = (size_t)t * N + m;
      const PnHdr* h = p.hdr + bm;
      const int npts = min(h->npts, V);
      if (npts <= 0) continue;                           // dead, or no finite vertex
      int x0, x1, y0, y1, z0, z1;
      const float cell = h->cell;
      const int dx = h->dim[0], dy = h->dim[1];
      if (!pn_axis(qx, rp, h->mn[0], h->mx[0], cell, dx, x0, x1) || !pn_axis(qy, rp, h->mn[1], h->mx[1], cell, dy, y0, y1) ||
          !pn_axis(qz, rp, h->mn[2], h->mx[2], cell, h->dim[2], z0, z1))
        continue;                                        // the box, grown by the radius, misses the query
      const int* st = p.start + bm * (PN_MAX_CELLS + 1);
      const uint4* sp = p.sorted + bm * V;
      const int base = m * V;
      for (int cz = z0; cz <= z1; ++cz)
        for (int cy = y0; cy <= y1; ++cy) {
          const int row = (cz * dy + cy) * dx;           // the cells of a row are consecutive: one run of the sorted vertices
          const int a = max(st[row + x0], 0), e = min(st[row + x1 + 1], npts);
          for (int k = a; k < e; ++k) {
            const uint4 s = sp[k];
            const float ex = __uint_as_float(s.x) - qx, ey = __uint_as_float(s.y) - qy, ez = __uint_as_float(s.z) - qz;
            const float d2 = (ex * ex + ey * ey) + ez * ez;
            if (!(d2 <= r2)) continue;                   // (NaN: no candidate)
            const int id = base + (int)min(s.w, (unsigned)(V - 1));
            if (d2 < bd || (d2 == bd && id < bi)) { bd = d2; bi = id; }
          }
        }
    }
  }
  if (p.d2) p.d2[i] = bd;
  if (p.idx) p.idx[i] = bi;
}

extern "C" size_t mh_person_nearest_bytes(int T, int N, int V) {
  return pn_bytes((size_t)(T > 0 ? T : 1) * (size_t)(N > 0 ? N : 1), (size_t)(V > 0 ? V : 1));
}

extern "C" int mh_person_nearest(int T, int N, int V, const float* verts, const uint8_t* live, float radius, void* ws, size_t ws_bytes,
                                 float* d2, int32_t* idx, void* stream) {
  MH_CHECK(T > 0 && N > 0 && V > 0, "empty input");
  MH_CHECK(N <= PN_MAX_N, "N must be at most 32 people per frame");
  MH_CHECK((long long)N * V <= 0x7fffffffll, "N * V must stay below 2^31: idx = m * V + u is an int32");
  MH_CHECK((long long)T * N * V <= PN_MAX_ITEMS, "too many vertices for one launch (T * N * V): call it on fewer frames");
  MH_CHECK(verts && ws, "null argument: verts and ws");
  MH_CHECK(ws_bytes >= mh_person_nearest_bytes(T, N, V), "workspace too small: ws_bytes is below mh_person_nearest_bytes(T, N, V)");
  MH_CHECK(d2 || idx, "no output requested (d2 and idx are both null)");
  MH_CHECK(radius > 0.f && radius < INFINITY, "radius must be finite and positive");
  MH_CHECK((double)radius <= PN_MAX_RADIUS, "radius too large: above 0.64 m, the cap of mh_scene_nearest");
  const int B = T * N, total = B * V;
  const unsigned nblk = (unsigned)((total + PN_BLOCK - 1) / PN_BLOCK);
  PnWs w = pn_carve(ws, (size_t)B, (size_t)V);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_pn_setup, dim3((unsigned)B), dim3(PN_BLOCK), 0, st, V, verts, live, w.hdr, w.start);
  MH_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_pn_count, dim3(nblk), dim3(PN_BLOCK), 0, st, total, V, verts, (const PnHdr*)w.hdr, w.start, w.pcell);
  MH_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_pn_scan, dim3((unsigned)B), dim3(1024), 0, st, (const PnHdr*)w.hdr, w.start, w.cursor);
  MH_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_pn_scatter, dim3(nblk), dim3(PN_BLOCK), 0, st, total, V, verts, (const int*)w.pcell, w.cursor, w.sorted);
  MH_LAUNCH_CHECK();
  PersonNearestP p;
  p.total = total; p.N = N; p.V = V; p.radius = radius;
  p.verts = verts; p.live = live;
  p.hdr = w.hdr; p.start = w.start; p.sorted = w.sorted;
  p.d2 = d2; p.idx = idx;
  hipLaunchKernelGGL(k_person_nearest, dim3(nblk), dim3(PN_BLOCK), 0, st, p);
  MH_LAUNCH_CHECK();
  return MH_OK;
}

// ---- vertex normals: a gather over the faces of every vertex ---------------------------------------------------------------
struct NormalsP {
  int total, V, F, A;
  const float* verts;
  const int* faces;
  const int* adj_start;
  const int* adj_face;
  float* normals;
};

__global__ __launch_bounds__(PN_BLOCK) void k_vertex_normals(NormalsP p) {
  const int i = blockIdx.x * PN_BLOCK + threadIdx.x;
  if (i >= p.total) return;
  const int b = i / p.V, v = i - b * p.V;
  const float* bv = p.verts + (size_t)b * p.V * 3;
  float nx = 0.f, ny = 0.f, nz = 0.f;
  const int k0 = max(p.adj_start[v], 0), k1 = min(p.adj_start[v + 1], p.A);
  for (int k = k0; k < k1; ++k) {                        // in the table's order: the sum has one value
    const int f = p.adj_face[k];
    if (f < 0 || f >= p.F) continue;
    const int i0 = p.faces[(size_t)f * 3], i1 = p.faces[(size_t)f * 3 + 1], i2 = p.faces[(size_t)f * 3 + 2];
    if (i0 < 0 || i0 >= p.V || i1 < 0 || i1 >= p.V || i2 < 0 || i2 >= p.V) continue;
    const float ax = bv[(size_t)i0 * 3], ay = bv[(size_t)i0 * 3 + 1], az = bv[(size_t)i0 * 3 + 2];
    const float e1x = bv[(size_t)i1 * 3] - ax, e1y = bv[(size_t)i1 * 3 + 1] - ay, e1z = bv[(size_t)i1 * 3 + 2] - az;
    const float e2x = bv[(size_t)i2 * 3] - ax, e2y = bv[(size_t)i2 * 3 + 1] - ay, e2z = bv[(size_t)i2 * 3 + 2] - az;
    nx = nx + (e1y * e2z - e1z * e2y);
    ny = ny + (e1z * e2x - e1x * e2z);
    nz = nz + (e1x * e2y - e1y * e2x);
  }
  p.normals[(size_t)i * 3] = nx;
  p.normals[(size_t)i * 3 + 1] = ny;
  p.normals[(size_t)i * 3 + 2] = nz;
}

extern "C" int mh_vertex_normals(int B, int V, int F, const float* verts, const int32_t* faces, const int32_t* adj_start,
                                 const int32_t* adj_face, int A, float* normals, void* stream) {
  MH_CHECK(B > 0 && V > 0 && F > 0, "empty input");
  MH_CHECK(A >= 0, "A (entries of adj_face) must not be negative");
  MH_CHECK((long long)B * V <= PN_MAX_ITEMS, "too many vertices for one launch (B * V)");
  MH_CHECK(verts && faces && adj_start && normals && (adj_face || A == 0), "null argument: verts, faces, adj_start, adj_face and normals");
  NormalsP p;
  p.total = B * V; p.V = V; p.F = F; p.A = A;
  p.verts = verts; p.faces = faces; p.adj_start = adj_start; p.adj_face = adj_face; p.normals = normals;
  hipLaunchKernelGGL(k_vertex_normals, dim3((unsigned)((p.total + PN_BLOCK - 1) / PN_BLOCK)), dim3(PN_BLOCK), 0, (hipStream_t)stream, p);
  MH_LAUNCH_CHECK();
  return MH_OK;
}

// ---- side test and the per-pair / per-part tables ---------------------------------------------------------------------------
struct PairsP {
  int N, V, P, bpb;                   // workgroups per body
  float thr2;
  const float* verts;
  const float* normals;
  const float* d2;
  const int* idx;
  const uint8_t* part;
  uint8_t* behind;
  int* pair_verts;
  unsigned* pair_min;                 // float bits: the values compared are >= 0, whose bits order like their values
  int* pair_behind;
  int* part_verts;
  unsigned long long* part_key;
};

__global__ __launch_bounds__(PN_BLOCK) void k_person_pairs(PairsP p) {
  __shared__ int s_pv[PN_MAX_N], s_pb[PN_MAX_N], s_cv[PN_MAX_N];
  __shared__ unsigned s_pm[PN_MAX_N];
  __shared__ unsigned long long s_key[PN_MAX_N];
  const int tid = threadIdx.x;
  const int b = blockIdx.x / p.bpb, v = (blockIdx.x - b * p.bpb) * PN_BLOCK + tid;      // b = t N + n
  const int N = p.N, V = p.V;
  if (tid < PN_MAX_N) { s_pv[tid] = 0; s_pb[tid] = 0; s_cv[tid] = 0; s_pm[tid] = PN_INF_BITS; s_key[tid] = ~0ull; }
  __syncthreads();
  if (v < V) {
    const size_t i = (size_t)b * V + v;
    const int id = p.idx[i];
    bool beh = false;
    if (id >= 0 && id / V < N) {                         // (an index beyond the frame's bodies is followed nowhere)
      const int m = id / V;
      const float d = p.d2[i];
      if (p.normals) {
        const size_t o = (size_t)(b / N) * N * V + id;   // vertex u of person m in the same frame
        const float qx = p.verts[i * 3], qy = p.verts[i * 3 + 1], qz = p.verts[i * 3 + 2];
        const float px = p.verts[o * 3], py = p.verts[o * 3 + 1], pz = p.verts[o * 3 + 2];
        const float wx = p.normals[o * 3], wy = p.normals[o * 3 + 1], wz = p.normals[o * 3 + 2];
        beh = ((qx - px) * wx + (qy - py) * wy) + (qz - pz) * wz < 0.f;
      }
      const bool touch = d <= p.thr2;
      const bool ranked = d >= 0.f;                      // NaN and negative values are never a minimum
      const unsigned dbits = __float_as_uint(d + 0.f);   // (-0 + 0 = +0)
      if (touch) {
        atomicAdd(&s_pv[m], 1);
        if (beh) atomicAdd(&s_pb[m], 1);
      }
      if (ranked) atomicMin(&s_pm[m], dbits);
      const int k = p.part[v];
      if (k < p.P) {
        if (touch) atomicAdd(&s_cv[k], 1);
        if (ranked) atomicMin(&s_key[k], ((unsigned long long)dbits << 32) | (unsigned)id);
      }
    }
    if (p.behind) p.behind[i] = beh ? 1 : 0;
  }
  __syncthreads();
  if (tid < N) {
    const size_t o = (size_t)b * N + tid;
    if (p.pair_verts && s_pv[tid] != 0) atomicAdd(&p.pair_verts[o], s_pv[tid]);
    if (p.pair_behind && s_pb[tid] != 0) atomicAdd(&p.pair_behind[o], s_pb[tid]);
    if (p.pair_min && s_pm[tid] != PN_INF_BITS) atomicMin(&p.pair_min[o], s_pm[tid]);
  }
  if (tid < p.P) {
    const size_t o = (size_t)b * p.P + tid;
    if (p.part_verts && s_cv[tid] != 0) atomicAdd(&p.part_verts[o], s_cv[tid]);
    if (p.part_key && s_key[tid] != ~0ull) atomicMin(&p.part_key[o], s_key[tid]);
  }
}

extern "C" int mh_person_pairs(int T, int N, int V, const float* verts, const float* normals, const float* d2, const int32_t* idx,
                               const uint8_t* part, int P, float thr, uint8_t* behind, int32_t* pair_verts, float* pair_min_d2,
                               int32_t* pair_behind, int32_t* part_verts, uint64_t* part_min_key, void* stream) {
  MH_CHECK(T > 0 && N > 0 && V > 0, "empty input");
  MH_CHECK(N <= PN_MAX_N, "N must be at most 32 people per frame");
  MH_CHECK(P >= 1 && P <= PN_MAX_N, "P must be in 1..32");
  MH_CHECK((long long)N * V <= 0x7fffffffll, "N * V must stay below 2^31: idx = m * V + u is an int32");
  MH_CHECK((long long)T * N * V <= PN_MAX_ITEMS, "too many vertices for one launch (T * N * V): call it on fewer frames");
  MH_CHECK(verts && d2 && idx && part, "null argument: verts, d2, idx and part");
  MH_CHECK(behind || pair_verts || pair_min_d2 || pair_behind || part_verts || part_min_key, "no output requested (every output is null)");
  MH_CHECK(thr >= 0.f && thr < INFINITY, "thr must be finite and not negative");
  PairsP p;
  p.N = N; p.V = V; p.P = P;
  p.bpb = (V + PN_BLOCK - 1) / PN_BLOCK;
  p.thr2 = thr * thr;
  p.verts = verts; p.normals = normals; p.d2 = d2; p.idx = idx; p.part = part;
  p.behind = behind; p.pair_verts = pair_verts; p.pair_min = (unsigned*)pair_min_d2; p.pair_behind = pair_behind;
  p.part_verts = part_verts; p.part_key = (unsigned long long*)part_min_key;
  const size_t B = (size_t)T * N;
  hipStream_t st = (hipStream_t)stream;
  if (pair_verts) MH_HIP(hipMemsetAsync(pair_verts, 0, B * N * sizeof(int32_t), st));
  if (pair_behind) MH_HIP(hipMemsetAsync(pair_behind, 0, B * N * sizeof(int32_t), st));
  if (pair_min_d2) MH_HIP(hipMemsetD32Async((hipDeviceptr_t)pair_min_d2, (int)PN_INF_BITS, B * N, st));
  if (part_verts) MH_HIP(hipMemsetAsync(part_verts, 0, B * P * sizeof(int32_t), st));
  if (part_min_key) MH_HIP(hipMemsetAsync(part_min_key, 0xff, B * P * sizeof(uint64_t), st));
  hipLaunchKernelGGL(k_person_pairs, dim3((unsigned)(B * p.bpb)), dim3(PN_BLOCK), 0, st, p);
  MH_LAUNCH_CHECK();
  return MH_OK;
}
