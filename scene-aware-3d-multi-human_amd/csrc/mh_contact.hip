// Body-to-scene contact map (mh_scene_nearest / mh_contact_parts, include/mhmocap_hip.h): for every vertex of every body the
// nearest point of the scene cloud within a radius, and per body and body part how many vertices touch the scene and how
// close the part comes.  Read-only on the grid mh_scene_grid_build[_dev] left; nothing of the fit's cycle is used.
//
// Nearest point: ONE LANE PER QUERY.  k_contact_knn_grid (mh_scene.hip) spends a wave and a 128-slot selection buffer on
// one query with k = 32 -- right for the 800 queries of a cycle, not for the 5.5 million vertices of a sequence.  With
// k = 1 and a radius the search needs no buffer and no shells: a lane walks the (z, y) rows of cells its box
// [q - r, q + r] touches; the cells of a row are consecutive in x, so the row's points are ONE run of the sorted cloud
// (start[first cell] .. start[last cell + 1]) and cost two loads of the cell table whatever the radius.
//
// The result is a function of the SET of candidates (smallest d2, ties by x, then y, then z), not of the order they are
// visited in, and the arithmetic is written in the order the header states and compiled without contraction: a float32
// evaluation of the same expressions on the host gives the same bits (tests/contact_ref.py).
#include "mh_common.h"
#include "mh_grid_p.h"

#include <math.h>

#pragma clang fp contract(off)

#define SN_BLOCK 256
#define SN_MIN_CELL 0.02            // the smallest cell k_grid_setup chooses (metres)
#define CP_BLOCK 256
#define CP_MAXP 32
#define CP_INF_BITS 0x7f800000u

struct NearestP {
  const GridHdr* hdr;
  const int* start;
  const float* sorted;
  const float* queries;
  int Q;
  float radius;
  float* d2;
  float* near_xyz;
};

// Cells [c0, c1] of one axis that can hold a candidate of a query at coordinate q; false: none can.
//
// Superset, by monotonicity.  A candidate has fl(fl(dx dx + dy dy) + dz dz) <= fl(r r) with dx = fl(p - q).  Rounding is
// monotone and the other two squares are >= 0, so fl(dx dx) <= fl(r r).  With rp = max(r (1 + 2^-20), 1e-12), |dx| >= rp
// would give dx dx >= r r (1 + 2^-20)^2, which no rounding brings back to fl(r r) <= r r (1 + 2^-24) (the floor of 1e-12 keeps
// rp rp a normal number where r r is not): every candidate has |fl(p - q)| < rp.
// L = the float below fl(q - rp) is <= q - rp in the reals (the step down is at least the half ulp the subtraction may
// have rounded up by).  A float p < L has p - q < -rp, hence fl(p - q) <= -rp: not a candidate.  So L <= p, and likewise
// p <= U = the float above fl(q + rp).
// The cell of a point is c(p) = clamp((int)fl(fl(p - mn) / cell), 0, dim - 1) (grid_cell): subtraction of a constant,
// division by a positive constant, truncation and clamping are all monotone, so c(L) <= c(p) <= c(U).  Below, f is
// clamped to [-1, dim] as a float first, which changes no result of the clamp to [0, dim - 1] and keeps the conversion
// in range for a query far outside.
// Miss: mn is the smallest coordinate of the cloud exactly, so U < mn (f(U) < 0) leaves no candidate; and every point
// has f(p) <= fl(extent / cell) < dim (dim = (int)fl(extent / cell) + 1 in k_grid_setup), so f(L) >= dim puts L above
// every point.
__device__ __forceinline__ bool sn_axis(float q, float rp, float mn, float cell, int dim, int& c0, int& c1) {
  const float L = nextafterf(q - rp, -INFINITY), U = nextafterf(q + rp, INFINITY);
  const float f0 = (L - mn) / cell, f1 = (U - mn) / cell;
  if (f1 < 0.f || f0 >= (float)dim) return false;
  c0 = min(max((int)fminf(fmaxf(f0, -1.f), (float)dim), 0), dim - 1);
  c1 = min(max((int)fminf(fmaxf(f1, -1.f), (float)dim), 0), dim - 1);
  return true;
}

__global__ __launch_bounds__(SN_BLOCK) void k_scene_nearest(NearestP p) {
  const int i = blockIdx.x * SN_BLOCK + threadIdx.x;
  if (i >= p.Q) return;
  const float qx = p.queries[(size_t)i * 3], qy = p.queries[(size_t)i * 3 + 1], qz = p.queries[(size_t)i * 3 + 2];
  float bd = INFINITY, bx = 0.f, by = 0.f, bz = 0.f;
  const int npts = p.hdr->npts;
  int x0 = 0, x1 = -1, y0 = 0, y1 = -1, z0 = 0, z1 = -1;
  const bool finite = fabsf(qx) < INFINITY && fabsf(qy) < INFINITY && fabsf(qz) < INFINITY;      // (false for NaN)
  if (npts > 0 && finite) {
    const float r2 = p.radius * p.radius;
    const float rp = fmaxf(p.radius * 1.000001f, 1e-12f);
    const float cell = p.hdr->cell;
    const int dx = p.hdr->dim[0], dy = p.hdr->dim[1], dz = p.hdr->dim[2];
    if (sn_axis(qx, rp, p.hdr->mn[0], cell, dx, x0, x1) && sn_axis(qy, rp, p.hdr->mn[1], cell, dy, y0, y1) &&
        sn_axis(qz, rp, p.hdr->mn[2], cell, dz, z0, z1)) {
      for (int cz = z0; cz <= z1; ++cz)
        for (int cy = y0; cy <= y1; ++cy) {
          const int row = (cz * dy + cy) * dx;
          // (the bounds of a built grid lie in [0, npts]; clamped so that a lane never leaves the sorted cloud)
          const int a = max(p.start[row + x0], 0), b = min(p.start[row + x1 + 1], npts);
          for (int k = a; k < b; ++k) {
            const float px = p.sorted[(size_t)k * 3], py = p.sorted[(size_t)k * 3 + 1], pz = p.sorted[(size_t)k * 3 + 2];
            const float ex = px - qx, ey = py - qy, ez = pz - qz;
            const float d2 = (ex * ex + ey * ey) + ez * ez;
            if (!(d2 <= r2)) continue;                                                           // (NaN: no candidate)
            if (d2 < bd || (d2 == bd && (px < bx || (px == bx && (py < by || (py == by && pz < bz)))))) {
              bd = d2; bx = px; by = py; bz = pz;
            }
          }
        }
    }
  }
  if (p.d2) p.d2[i] = bd;
  if (p.near_xyz) {
    p.near_xyz[(size_t)i * 3] = bx;
    p.near_xyz[(size_t)i * 3 + 1] = by;
    p.near_xyz[(size_t)i * 3 + 2] = bz;
  }
}

extern "C" int mh_scene_nearest(const void* grid_ws, int M, const float* queries, int Q, float radius, float* d2,
                                float* near_xyz, void* stream) {
  MH_CHECK(Q > 0 && M > 0, "empty input");
  MH_CHECK(Q <= 0x7fffffff - SN_BLOCK, "too many queries for one launch");
  MH_CHECK(grid_ws && queries, "null argument: grid_ws and queries");
  MH_CHECK(d2 || near_xyz, "no output requested (d2 and near_xyz are both null)");
  MH_CHECK(radius > 0.f && radius < INFINITY, "radius must be finite and positive");
  MH_CHECK((double)radius <= MH_SCENE_NEAREST_MAX_CELLS * SN_MIN_CELL,
           "radius too large: more than MH_SCENE_NEAREST_MAX_CELLS of the smallest cell (0.02 m)");
  GridWs g = grid_carve((void*)grid_ws, M);
  NearestP p;
  p.hdr = g.hdr; p.start = g.start; p.sorted = g.sorted;
  p.queries = queries; p.Q = Q; p.radius = radius;
  p.d2 = d2; p.near_xyz = near_xyz;
  hipLaunchKernelGGL(k_scene_nearest, dim3((unsigned)((Q + SN_BLOCK - 1) / SN_BLOCK)), dim3(SN_BLOCK), 0, (hipStream_t)stream, p);
  MH_LAUNCH_CHECK();
  return MH_OK;
}

// ---- per body and part --------------------------------------------------------------------------------------------------------
struct PartsP {
  int V, P, bpb;                      // workgroups per body
  float thr2;
  const float* d2;
  const uint8_t* part;
  int* counts;
  unsigned* min_d2;                   // float bits: the values compared are >= 0, whose bits order like their values
};

__global__ __launch_bounds__(CP_BLOCK) void k_contact_parts(PartsP p) {
  __shared__ int s_cnt[CP_MAXP];
  __shared__ unsigned s_min[CP_MAXP];
  const int tid = threadIdx.x;
  const int b = blockIdx.x / p.bpb, v = (blockIdx.x - b * p.bpb) * CP_BLOCK + tid;
  if (tid < CP_MAXP) { s_cnt[tid] = 0; s_min[tid] = CP_INF_BITS; }
  __syncthreads();
  if (v < p.V) {
    const int k = p.part[v];
    const float d = p.d2[(size_t)b * p.V + v];
    if (k < p.P) {
      if (d <= p.thr2) atomicAdd(&s_cnt[k], 1);
      if (d >= 0.f && d < INFINITY) atomicMin(&s_min[k], __float_as_uint(d + 0.f));       // (-0 + 0 = +0)
    }
  }
  __syncthreads();
  if (tid < p.P) {
    if (p.counts && s_cnt[tid] != 0) atomicAdd(&p.counts[(size_t)b * p.P + tid], s_cnt[tid]);
    if (p.min_d2 && s_min[tid] != CP_INF_BITS) atomicMin(&p.min_d2[(size_t)b * p.P + tid], s_min[tid]);
  }
}

extern "C" int mh_contact_parts(int B, int V, const float* d2, const uint8_t* part, int P, float thr, int32_t* counts,
                                float* min_d2, void* stream) {
  MH_CHECK(B > 0 && V > 0, "empty input");
  MH_CHECK(P >= 1 && P <= CP_MAXP, "P must be in 1..32");
  MH_CHECK(d2 && part, "null argument: d2 and part");
  MH_CHECK(counts || min_d2, "no output requested (counts and min_d2 are both null)");
  MH_CHECK(thr >= 0.f && thr < INFINITY, "thr must be finite and not negative");
  PartsP p;
  p.V = V; p.P = P;
  p.bpb = (V + CP_BLOCK - 1) / CP_BLOCK;
  MH_CHECK((long long)B * p.bpb <= 0x7fffffffll, "too many bodies for one launch");
  p.thr2 = thr * thr;
  p.d2 = d2; p.part = part;
  p.counts = counts; p.min_d2 = (unsigned*)min_d2;
  hipStream_t st = (hipStream_t)stream;
  if (counts) MH_HIP(hipMemsetAsync(counts, 0, (size_t)B * P * sizeof(int32_t), st));
  if (min_d2) MH_HIP(hipMemsetD32Async((hipDeviceptr_t)min_d2, (int)CP_INF_BITS, (size_t)B * P, st));
  hipLaunchKernelGGL(k_contact_parts, dim3((unsigned)(B * p.bpb)), dim3(CP_BLOCK), 0, st, p);
  MH_LAUNCH_CHECK();
  return MH_OK;
}
