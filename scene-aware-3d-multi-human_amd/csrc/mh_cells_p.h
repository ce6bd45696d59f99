// What the cell lists of the library share: the grid over the scene cloud (mh_grid_p.h, mh_scene.hip), the vertex grid per body
// (mh_proximity.hip) and the two face grids per body (mh_inside.hip, mh_surface.hip) are all built as "box, count, exclusive
// scan, fill" over a workspace of one layout.  Internal to the library (not part of the C ABI).  Integer and min / max code
// only: nothing here depends on the floating-point contraction setting of the file that includes it.
//
// Each file keeps what differs: its header struct, the rule that shapes its grid, its record, its cell function, its visit.
#pragma once
#include "mh_common.h"

static size_t cells_align(size_t x) { return (x + 255) & ~(size_t)255; }

// ---- the workspace: headers [B], start [B][C + 1], cursor [B][C], and two payload arrays of a and b bytes ------------------------
struct CellsWs {
  void* hdr;
  int* start;
  int* cursor;
  void* a;
  void* b;
};
static size_t cells_bytes(size_t B, size_t hdr_size, size_t C, size_t a_bytes, size_t b_bytes) {
  return cells_align(B * hdr_size) + cells_align(B * (C + 1) * 4) + cells_align(B * C * 4) + cells_align(a_bytes) + cells_align(b_bytes);
}
static CellsWs cells_carve(void* ws, size_t B, size_t hdr_size, size_t C, size_t a_bytes) {
  char* c = (char*)ws;
  CellsWs w;
  w.hdr = c; c += cells_align(B * hdr_size);
  w.start = (int*)c; c += cells_align(B * (C + 1) * 4);
  w.cursor = (int*)c; c += cells_align(B * C * 4);
  w.a = c; c += cells_align(a_bytes);
  w.b = c;
  return w;
}

// ---- the box of a workgroup: shuffles inside the waves, one LDS hop for the wave results -------------------------------------------
__device__ __forceinline__ float cells_min(float a, float b) { return fminf(a, b); }
__device__ __forceinline__ float cells_max(float a, float b) { return fmaxf(a, b); }
__device__ __forceinline__ int cells_min(int a, int b) { return min(a, b); }
__device__ __forceinline__ int cells_max(int a, int b) { return max(a, b); }

// Every thread of the workgroup of THREADS brings its own mn / mx; on return thread 0 holds the workgroup's.  Contains a
// barrier (after the caller's own writes to LDS, which it so publishes as well): call it from uniform code.
template <int THREADS, class T>
__device__ __forceinline__ void cells_box_reduce(T mn[3], T mx[3]) {
  __shared__ T smn[3][THREADS / 64], smx[3][THREADS / 64];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      mn[c] = cells_min(mn[c], __shfl_xor(mn[c], o, 64));
      mx[c] = cells_max(mx[c], __shfl_xor(mx[c], o, 64));
    }
    if ((threadIdx.x & 63) == 0) { smn[c][threadIdx.x >> 6] = mn[c]; smx[c][threadIdx.x >> 6] = mx[c]; }
  }
  __syncthreads();
  if (threadIdx.x == 0)
    for (int c = 0; c < 3; ++c)
      for (int w = 1; w < THREADS / 64; ++w) { mn[c] = cells_min(mn[c], smn[c][w]); mx[c] = cells_max(mx[c], smx[c][w]); }
}

// ---- the scan: counts[0..nc] of one body, exclusive and in place, copied to the fill cursors -----------------------------------------
// A workgroup of 1024 threads: DPP scan inside the waves, one LDS hop for the 16 wave totals, a carry from pass to pass of
// 1024 cells.  Contains barriers: every thread of the workgroup calls it, after the kernel's uniform early-outs.
__device__ __forceinline__ void cells_scan_1024(int nc, int* counts, int* cursor) {
  __shared__ int swave[16];
  __shared__ int carry;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (threadIdx.x == 0) carry = 0;
  __syncthreads();
  for (int base = 0; base < nc; base += 1024) {
    const int i = base + threadIdx.x;
    const int v = i < nc ? counts[i] : 0;
    const int incl = mh_wave_scan_add(v);
    if (lane == 63) swave[wave] = incl;
    __syncthreads();
    int woff = carry;
#pragma unroll
    for (int w = 0; w < 16; ++w) woff += (w < wave) ? swave[w] : 0;
    if (i < nc) {
      const int start = woff + incl - v;
      counts[i] = start;
      cursor[i] = start;
    }
    __syncthreads();
    if (threadIdx.x == 1023) carry = woff + incl;
    __syncthreads();
  }
  if (threadIdx.x == 0) counts[nc] = carry;
}

// ---- the two face grids: faces listed by cell ----------------------------------------------------------------------------------------
// A grid G names what differs:  Hdr (with int flags: 0 = the body's lists are filled; unsigned long long total),  Rec (three per
// face, the corners),  BLOCK, MAX_CELLS, CAP_PER_FACE,  counted(h, F, force): the body takes the grid path,  valid(first Rec),
// range(h, three Recs, c0[3], c1[3]): the cells the face overlaps,  cell(h, cx, cy, cz): the index of one.

// a body whose lists would need more than cap_per_face entries per face has none: its queries walk all faces
__device__ __forceinline__ bool cells_over_cap(unsigned long long total, int F, int cap_per_face) {
  return total > (unsigned long long)cap_per_face * (unsigned long long)F;
}

// the workgroups of a body are consecutive, fpb of them: body and face of this lane
template <int BLOCK>
__device__ __forceinline__ int cells_body_face(int fpb, size_t& b) {
  b = blockIdx.x / fpb;
  return (int)(blockIdx.x - b * fpb) * BLOCK + threadIdx.x;
}

// face f in every cell of its range: counted in table (lst null), or entered in lst at the cell's cursor in table
template <class G>
__device__ __forceinline__ void cells_face_walk(const typename G::Hdr& h, int F, const typename G::Rec* r, int f, int* table, int* lst) {
  const typename G::Rec p0 = r[0], p1 = r[1], p2 = r[2];
  if (!G::valid(p0)) return;
  int c0[3], c1[3];
  G::range(h, p0, p1, p2, c0, c1);
  const long long cap = (long long)F * G::CAP_PER_FACE;
  for (int cz = c0[2]; cz <= c1[2]; ++cz)
    for (int cy = c0[1]; cy <= c1[1]; ++cy)
      for (int cx = c0[0]; cx <= c1[0]; ++cx) {
        const int pos = atomicAdd(&table[G::cell(h, cx, cy, cz)], 1);
        if (lst && pos >= 0 && pos < cap) lst[pos] = f;    // (cannot miss after the count; a lane never leaves its body's slab)
      }
}

// one lane per (body, face): the face counted in every cell of its range (grid-path bodies only: at most CAP_PER_FACE F atomics a body)
template <class G>
__global__ __launch_bounds__(G::BLOCK) void k_cells_count(int F, int fpb, int force, const typename G::Hdr* hdrs, const typename G::Rec* rec,
                                                          int* start) {
  size_t b;
  const int f = cells_body_face<G::BLOCK>(fpb, b);
  if (f >= F) return;
  const typename G::Hdr h = hdrs[b];
  if (!G::counted(h, F, force)) return;
  cells_face_walk<G>(h, F, rec + (b * F + f) * 3, f, start + b * (G::MAX_CELLS + 1), nullptr);
}

template <class G>
__global__ __launch_bounds__(G::BLOCK) void k_cells_fill(int F, int fpb, const typename G::Hdr* hdrs, const typename G::Rec* rec, int* cursor,
                                                         int* list) {
  size_t b;
  const int f = cells_body_face<G::BLOCK>(fpb, b);
  if (f >= F) return;
  const typename G::Hdr h = hdrs[b];
  if (h.flags != 0) return;                                // dead, not testable, or walking all faces
  cells_face_walk<G>(h, F, rec + (b * F + f) * 3, f, cursor + b * G::MAX_CELLS, list + b * (size_t)F * G::CAP_PER_FACE);
}

// the query's read of cell c: visit(f) for the faces listed there, clamped so that nothing a table holds leads out of the lists
template <class Visit>
__device__ __forceinline__ void cells_visit(const int* __restrict__ start, const int* __restrict__ list, int c, int F, int cap_per_face,
                                            Visit visit) {
  const long long cap = (long long)F * cap_per_face;
  const int a = max(start[c], 0);
  const int e = (int)min((long long)start[c + 1], cap);
  for (int k = a; k < e; ++k) {
    const int f = list[k];
    if ((unsigned)f < (unsigned)F) visit(f);
  }
}
