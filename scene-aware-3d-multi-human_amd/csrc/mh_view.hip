// Free-viewpoint render of a fit (mh_view_project / _clear / _raster / _splat / _resolve, include/mhmocap_hip.h): the fitted
// meshes and the coloured scene point cloud drawn from ANY camera into one hard z-buffer.  Beside the hot path: it reads
// vertices and points, owns its buffers and shares nothing with the rasteriser of the fit (mh_raster.hip), whose selection
// pass is specialised for the fit camera (fixed znear / zfar, soft-silhouette windows, face sort state, float near-ties).
//
// ALL-INTEGER after the projection.  Vertices and points are projected once in float32 and snapped to fixed point; coverage,
// depth interpolation and the depth test are integer arithmetic and the z-buffer is ONE 64-bit unsigned atomic minimum per
// covered pixel in device memory.  A minimum over integers is exact in any order: the images have the same bits on every
// launch and equal a numpy restatement (tests/view_ref.py) bit for bit.
//
// Conventions
//   screen   1/64 pixel: xq = rint(u * 64), yq = rint(v * 64), u = fx xc / zc + cx, v = fy yc / zc + cy,
//            (xc, yc, zc) = R X + t in float32 (x right, y down, z forward: the fit's camera convention).
//            Pixel (px, py) has its centre at (64 px + 32, 64 py + 32).
//   depth    zq = rint(zc * 4096), units of 2^-12 m; valid 1 <= zq < 2^20 (everything from 256 m on is invalid).
//   validity a vertex or point is INVALID if zc < near (or zc is NaN), if zq is outside its range or if |xq| or |yq| >= 2^18
//            (a guard band of +-4096 px).  It is written as (INT32_MIN, 0, 0).  W, H <= 4096.
//   faces    a face with an invalid vertex is DROPPED.  FACES ARE NOT CLIPPED: a face that crosses the near plane or leaves
//            the guard band disappears as a whole (the reference's viewer clips; bodies here stand in front of the camera).
//            Both windings are drawn, a face of zero area is skipped.  With E0, E1, E2 the integer edge functions at a
//            pixel centre (E_i opposite vertex i), signed so that their sum A (twice the area, units^2) is positive, the
//            pixel is covered iff E0, E1, E2 >= 0 -- edges are inclusive, a shared edge is covered by both faces and the key
//            decides -- and its depth is zpix = (E0 z0 + E1 z1 + E2 z2) // A in int64.  Bound: coordinate differences are
//            below 2^19, so |E_i| < 2^39 and every product E_i z_i < 2^59: the sum of three stays below 2^61.
//   points   a point covers the square of 2 half + 1 pixels around the pixel (xq >> 6, yq >> 6) that contains it, clipped
//            to the image, every pixel at depth zq; half = min(max_half, (size_q * fq // zq) // 128) with size_q =
//            rint(size_m * 4096) the point's extent in metres (negative: 0), fq = rint(fx * 64), max_half <= 8.
//   key      (uint64) zpix << 32 | payload; payload = n F + f for face f of person n, 0x80000000 | index for a point: at an
//            exact depth tie a mesh beats the scene, a lower person a higher one, a lower point index a higher one.
//            Empty = all ones.
#include "mh_common.h"

#define VW_BLOCK 256
#define VW_MAXN 32
#define VW_MAXVIEWS 64
#define VW_MAXDIM 4096
#define VW_MAXHALF 8
#define VW_WIDE 16                    // pixels in a face's clipped box above which the wave draws it together
#define VW_EMPTY 0xffffffffffffffffull
#define VW_INVALID INT32_MIN
#define VW_POINT 0x80000000u

// ---- projection ---------------------------------------------------------------------------------------------------------------
struct ViewCams { float m[VW_MAXVIEWS][12]; };        // per view: R row-major, then t (3 KB of kernel arguments)

struct ViewProjectP {
  int count, per_view;
  float fx, fy, cx, cy, near;
  const float* xyz;
  int* out;
};

__global__ __launch_bounds__(VW_BLOCK) void k_view_project(ViewProjectP p, ViewCams cams) {
  const int i = blockIdx.x * VW_BLOCK + threadIdx.x;
  if (i >= p.count) return;
  const int v = blockIdx.y;
  const float* c = cams.m[v];
  const size_t orow = (size_t)v * p.count + i, irow = p.per_view ? orow : (size_t)i;
  const float X = p.xyz[irow * 3], Y = p.xyz[irow * 3 + 1], Z = p.xyz[irow * 3 + 2];
  const float xc = c[0] * X + c[1] * Y + c[2] * Z + c[9];
  const float yc = c[3] * X + c[4] * Y + c[5] * Z + c[10];
  const float zc = c[6] * X + c[7] * Y + c[8] * Z + c[11];
  int xq = VW_INVALID, yq = 0, zq = 0;
  if (zc >= p.near) {                                  // (false for NaN)
    const float zf = rintf(zc * 4096.f);
    const float uf = rintf((p.fx * xc / zc + p.cx) * 64.f), vf = rintf((p.fy * yc / zc + p.cy) * 64.f);
    // the ranges are checked on the floats: nothing out of range (or NaN) is converted
    if (zf >= 1.f && zf < 1048576.f && fabsf(uf) < 262144.f && fabsf(vf) < 262144.f) { xq = (int)uf; yq = (int)vf; zq = (int)zf; }
  }
  int* o = p.out + orow * 3;
  o[0] = xq; o[1] = yq; o[2] = zq;
}

extern "C" int mh_view_project(int count, int per_view, int Tv, const float* xyz, const float* R, const float* t, const float* K,
                               float near, int32_t* out_q, void* stream) {
  MH_CHECK(count > 0 && Tv > 0, "empty input");
  MH_CHECK(Tv <= VW_MAXVIEWS, "more than 64 views in one call (the cameras travel as kernel arguments)");
  MH_CHECK(per_view == 0 || per_view == 1, "per_view must be 0 or 1");
  MH_CHECK(xyz && R && t && K && out_q, "null argument");
  MH_CHECK(near > 0.f, "near must be positive");         // (false for NaN)
  MH_CHECK(count <= 0x7fffffff - VW_BLOCK, "too many entries for one launch");
  ViewProjectP p;
  p.count = count; p.per_view = per_view;
  p.fx = K[0]; p.cx = K[2]; p.fy = K[4]; p.cy = K[5];
  p.near = near;
  p.xyz = xyz; p.out = out_q;
  ViewCams cams;
  memset(&cams, 0, sizeof(cams));
  for (int v = 0; v < Tv; ++v) {
    memcpy(cams.m[v], R + (size_t)v * 9, 9 * sizeof(float));
    memcpy(cams.m[v] + 9, t + (size_t)v * 3, 3 * sizeof(float));
  }
  hipLaunchKernelGGL(k_view_project, dim3((unsigned)((count + VW_BLOCK - 1) / VW_BLOCK), (unsigned)Tv), dim3(VW_BLOCK), 0,
                     (hipStream_t)stream, p, cams);
  MH_LAUNCH_CHECK();
  return MH_OK;
}

// ---- z-buffer -----------------------------------------------------------------------------------------------------------------
extern "C" int mh_view_clear(int T, int H, int W, uint64_t* keys, void* stream) {
  MH_CHECK(T > 0 && H > 0 && W > 0, "empty input");
  MH_CHECK(H <= VW_MAXDIM && W <= VW_MAXDIM, "image larger than 4096 x 4096");
  MH_CHECK(keys, "null argument");
  MH_HIP(hipMemsetAsync(keys, 0xff, (size_t)T * H * W * sizeof(uint64_t), (hipStream_t)stream));
  return MH_OK;
}

struct ViewRasterP {
  int T, N, V, F, H, W;
  long long total;                    // T N F
  const int* vq;
  const int* faces;
  unsigned long long* keys;
};

// edge function of a -> b at p: > 0 on one side, 0 on the line (differences below 2^19: the products need 64 bits)
__device__ __forceinline__ long long vw_edge(int ax, int ay, int bx, int by, int px, int py) {
  return (long long)(bx - ax) * (py - ay) - (long long)(by - ay) * (px - ax);
}

// the depth test of pixel (px, py) of frame-image `img` against one face; A != 0 is the face's signed double area
__device__ __forceinline__ void vw_face_pixel(int x0, int y0, int z0, int x1, int y1, int z1, int x2, int y2, int z2, long long A,
                                              int px, int py, int W, unsigned payload, unsigned long long* img) {
  const int qx = px * 64 + 32, qy = py * 64 + 32;
  long long e0 = vw_edge(x1, y1, x2, y2, qx, qy), e1 = vw_edge(x2, y2, x0, y0, qx, qy), e2 = vw_edge(x0, y0, x1, y1, qx, qy);
  if (A < 0) { e0 = -e0; e1 = -e1; e2 = -e2; A = -A; }
  if ((e0 | e1 | e2) < 0) return;                      // (the sign bit of the OR: one of them is negative)
  const unsigned long long num = (unsigned long long)(e0 * z0 + e1 * z1 + e2 * z2);      // < 2^61, see the header comment
  const unsigned long long z = num / (unsigned long long)A;
  atomicMin(&img[(size_t)py * W + px], z << 32 | payload);
}

// One lane per face.  An SMPL face at 240x135 covers 0 to 4 pixels: a lane walks the pixels of its clipped box itself when
// they are at most VW_WIDE, in ONE flattened loop (the lanes of a wave then differ by at most VW_WIDE short iterations).  A
// face with a larger box is handed to the whole wave afterwards: its nine coordinates go round by shuffles and the 64 lanes
// stride over the box, so one full-image triangle costs box / 64 iterations and does not serialise the launch behind a lane.
__global__ __launch_bounds__(VW_BLOCK) void k_view_raster(ViewRasterP p) {
  const int lane = threadIdx.x & 63;
  const long long g = (long long)blockIdx.x * VW_BLOCK + threadIdx.x;       // (no early return: every lane takes part in the shuffles)
  int x0 = 0, y0 = 0, z0 = 0, x1 = 0, y1 = 0, z1 = 0, x2 = 0, y2 = 0, z2 = 0;
  int bx0 = 0, by0 = 0, bw = 0, bh = 0, t = 0;
  unsigned payload = 0u;
  long long A = 0;
  if (g < p.total) {
    const int NF = p.N * p.F;
    t = (int)(g / NF);
    const int r = (int)(g - (long long)t * NF);        // = n F + f: the payload
    const int n = r / p.F, f = r - n * p.F;
    payload = (unsigned)r;
    const int i0 = p.faces[f * 3], i1 = p.faces[f * 3 + 1], i2 = p.faces[f * 3 + 2];
    if ((unsigned)i0 < (unsigned)p.V && (unsigned)i1 < (unsigned)p.V && (unsigned)i2 < (unsigned)p.V) {
      const int* vb = p.vq + ((size_t)t * p.N + n) * p.V * 3;
      x0 = vb[i0 * 3]; y0 = vb[i0 * 3 + 1]; z0 = vb[i0 * 3 + 2];
      x1 = vb[i1 * 3]; y1 = vb[i1 * 3 + 1]; z1 = vb[i1 * 3 + 2];
      x2 = vb[i2 * 3]; y2 = vb[i2 * 3 + 1]; z2 = vb[i2 * 3 + 2];
      if (x0 != VW_INVALID && x1 != VW_INVALID && x2 != VW_INVALID) {
        A = vw_edge(x0, y0, x1, y1, x2, y2);
        // pixels whose centre 64 px + 32 lies in [min, max], clipped to the image (>> is the floor for negative values too)
        bx0 = max(0, (min(x0, min(x1, x2)) - 32 + 63) >> 6);
        by0 = max(0, (min(y0, min(y1, y2)) - 32 + 63) >> 6);
        const int bx1 = min(p.W - 1, (max(x0, max(x1, x2)) - 32) >> 6);
        const int by1 = min(p.H - 1, (max(y0, max(y1, y2)) - 32) >> 6);
        bw = bx1 - bx0 + 1; bh = by1 - by0 + 1;
      }
    }
  }
  const bool draw = A != 0 && bw > 0 && bh > 0;
  const int area = draw ? bw * bh : 0;                 // <= 4096 x 4096
  unsigned long long* img = p.keys + (size_t)t * p.H * p.W;
  if (area <= VW_WIDE) {
    int px = bx0, py = by0;
    for (int k = 0; k < area; ++k) {
      vw_face_pixel(x0, y0, z0, x1, y1, z1, x2, y2, z2, A, px, py, p.W, payload, img);
      if (++px == bx0 + bw) { px = bx0; ++py; }
    }
  }
  unsigned long long wide = __ballot(area > VW_WIDE);
  while (wide) {                                       // (wave-uniform)
    const int s = __ffsll((long long)wide) - 1;
    wide &= wide - 1ull;
    const int sx0 = __shfl(x0, s, 64), sy0 = __shfl(y0, s, 64), sz0 = __shfl(z0, s, 64);
    const int sx1 = __shfl(x1, s, 64), sy1 = __shfl(y1, s, 64), sz1 = __shfl(z1, s, 64);
    const int sx2 = __shfl(x2, s, 64), sy2 = __shfl(y2, s, 64), sz2 = __shfl(z2, s, 64);
    const int sbx = __shfl(bx0, s, 64), sby = __shfl(by0, s, 64), sbw = __shfl(bw, s, 64), sarea = __shfl(area, s, 64);
    const int st = __shfl(t, s, 64);
    const unsigned spay = (unsigned)__shfl((int)payload, s, 64);
    const long long sA = vw_edge(sx0, sy0, sx1, sy1, sx2, sy2);
    unsigned long long* simg = p.keys + (size_t)st * p.H * p.W;
    for (int k = lane; k < sarea; k += 64) {
      const int ry = k / sbw;
      vw_face_pixel(sx0, sy0, sz0, sx1, sy1, sz1, sx2, sy2, sz2, sA, sbx + (k - ry * sbw), sby + ry, p.W, spay, simg);
    }
  }
}

extern "C" int mh_view_raster(int T, int N, int V, int F, int H, int W, const int32_t* vq, const int32_t* faces, uint64_t* keys,
                              void* stream) {
  MH_CHECK(T > 0 && N > 0 && V > 0 && F > 0 && H > 0 && W > 0, "empty input");
  MH_CHECK(N <= VW_MAXN, "more than 32 people per frame");
  MH_CHECK(H <= VW_MAXDIM && W <= VW_MAXDIM, "image larger than 4096 x 4096");
  MH_CHECK((long long)N * F < 0x80000000ll, "N F must be below 2^31 (person and face share the key's low word with the points)");
  MH_CHECK((long long)T * N * F <= 0x7fffffffll * VW_BLOCK, "too many faces for one launch");
  MH_CHECK(vq && faces && keys, "null argument");
  ViewRasterP p;
  p.T = T; p.N = N; p.V = V; p.F = F; p.H = H; p.W = W;
  p.total = (long long)T * N * F;
  p.vq = vq; p.faces = faces; p.keys = (unsigned long long*)keys;
  hipLaunchKernelGGL(k_view_raster, dim3((unsigned)((p.total + VW_BLOCK - 1) / VW_BLOCK)), dim3(VW_BLOCK), 0, (hipStream_t)stream, p);
  MH_LAUNCH_CHECK();
  return MH_OK;
}

struct ViewSplatP {
  int T, P, H, W, fq, max_half;
  const int* pq;
  const int* size_q;
  unsigned long long* keys;
};

// One lane per point and frame; the (2 half + 1)^2 <= 289 pixels of its clipped square in one flattened loop.
__global__ __launch_bounds__(VW_BLOCK) void k_view_splat(ViewSplatP p) {
  const int i = blockIdx.x * VW_BLOCK + threadIdx.x, t = blockIdx.y;
  if (i >= p.P) return;
  const int* q = p.pq + ((size_t)t * p.P + i) * 3;
  const int xq = q[0], yq = q[1], zq = q[2];
  if (xq == VW_INVALID || zq < 1) return;
  const int sq = max(p.size_q ? p.size_q[i] : 0, 0);
  const int half = (int)min((long long)p.max_half, ((long long)sq * p.fq / zq) >> 7);
  const int px = xq >> 6, py = yq >> 6;                // the pixel that contains the point (floor)
  const int bx0 = max(0, px - half), by0 = max(0, py - half);
  const int bw = min(p.W - 1, px + half) - bx0 + 1, bh = min(p.H - 1, py + half) - by0 + 1;
  if (bw <= 0 || bh <= 0) return;
  const unsigned long long key = (unsigned long long)zq << 32 | (VW_POINT | (unsigned)i);
  unsigned long long* img = p.keys + (size_t)t * p.H * p.W;
  int x = bx0, y = by0;
  for (int k = 0; k < bw * bh; ++k) {
    atomicMin(&img[(size_t)y * p.W + x], key);
    if (++x == bx0 + bw) { x = bx0; ++y; }
  }
}

extern "C" int mh_view_splat(int T, int P, int H, int W, const int32_t* pq, const int32_t* size_q, int fq, int max_half,
                             uint64_t* keys, void* stream) {
  MH_CHECK(T > 0 && P > 0 && H > 0 && W > 0, "empty input");
  MH_CHECK(T <= 65535, "more than 65535 frames in one call (frames are the grid's second dimension)");
  MH_CHECK(H <= VW_MAXDIM && W <= VW_MAXDIM, "image larger than 4096 x 4096");
  MH_CHECK(max_half >= 0 && max_half <= VW_MAXHALF, "max_half must be in [0, 8]");
  MH_CHECK(fq > 0, "fq (the view's focal length in 1/64 pixel) must be positive");
  MH_CHECK(P <= 0x7fffffff - VW_BLOCK, "too many points (the index shares the key's low word with the mesh flag)");
  MH_CHECK(pq && keys, "null argument");
  ViewSplatP p;
  p.T = T; p.P = P; p.H = H; p.W = W; p.fq = fq; p.max_half = max_half;
  p.pq = pq; p.size_q = size_q; p.keys = (unsigned long long*)keys;
  hipLaunchKernelGGL(k_view_splat, dim3((unsigned)((P + VW_BLOCK - 1) / VW_BLOCK), (unsigned)T), dim3(VW_BLOCK), 0,
                     (hipStream_t)stream, p);
  MH_LAUNCH_CHECK();
  return MH_OK;
}

// ---- keys -> images -----------------------------------------------------------------------------------------------------------
struct ViewResolveP {
  int T, N, V, F, H, W;
  const unsigned long long* keys;
  const float* verts;
  const int* faces;
  const uint8_t* point_rgb;
  const float* palette;
  float lx, ly, lz, ambient;
  unsigned bg;                        // r | g << 8 | b << 16
  uint8_t* image;
  float* depth;
  int* label;
  int* face;
  int* coverage;
};

// (the compensated products and the rounding of mh_scene_composite, mh_render.hip: the same shade from the same vertices)
__device__ __forceinline__ float vw_diff_of_products(float a, float b, float c, float d) {
  const float w = c * d;
  const float e = fmaf(-c, d, w);
  const float f = fmaf(a, b, -w);
  return f + e;
}

__device__ __forceinline__ unsigned vw_u8(float v) {
  return (unsigned)__float2int_rn(fminf(fmaxf(v, 0.f), 255.f));
}

// One lane per pixel, frames across the grid's y: 8 bytes in, up to 19 out.
__global__ __launch_bounds__(VW_BLOCK) void k_view_resolve(ViewResolveP p) {
  __shared__ int s_cov[VW_MAXN + 1];
  const int tid = threadIdx.x, lane = tid & 63;
  const int t = blockIdx.y, P = p.H * p.W;
  const int i = blockIdx.x * VW_BLOCK + tid;
  const bool inside = i < P;
  if (p.coverage && tid <= VW_MAXN) s_cov[tid] = 0;
  if (p.coverage) __syncthreads();
  const size_t gp = (size_t)t * P + i;
  const unsigned long long key = inside ? p.keys[gp] : VW_EMPTY;
  const unsigned pay = (unsigned)key;
  int who = -1, idx = -1;             // who: person, N = scene, -1 = empty (a key no draw call can have written counts as empty)
  if (key != VW_EMPTY) {
    if (pay & VW_POINT) { who = p.N; idx = (int)(pay & ~VW_POINT); }
    else if (pay / (unsigned)p.F < (unsigned)p.N) { who = (int)(pay / (unsigned)p.F); idx = (int)(pay - (unsigned)who * (unsigned)p.F); }
  }
  if (inside) {
    if (p.depth) p.depth[gp] = who >= 0 ? (float)(unsigned)(key >> 32) * (1.f / 4096.f) : -1.f;      // < 2^20: exact
    if (p.label) p.label[gp] = who < 0 ? -1 : (who == p.N ? -2 : who);
    if (p.face) p.face[gp] = idx;
    if (p.image) {
      unsigned out = p.bg;
      if (who == p.N) {
        out = 128u | 128u << 8 | 128u << 16;
        if (p.point_rgb) { const uint8_t* c = p.point_rgb + (size_t)idx * 3; out = (unsigned)c[0] | (unsigned)c[1] << 8 | (unsigned)c[2] << 16; }
      } else if (who >= 0) {
        float nx = 0.f, ny = 0.f, nz = 0.f;
        const int i0 = p.faces[idx * 3], i1 = p.faces[idx * 3 + 1], i2 = p.faces[idx * 3 + 2];
        if ((unsigned)i0 < (unsigned)p.V && (unsigned)i1 < (unsigned)p.V && (unsigned)i2 < (unsigned)p.V) {
          const float* vb = p.verts + ((size_t)t * p.N + who) * p.V * 3;
          const float ax = vb[i0 * 3], ay = vb[i0 * 3 + 1], az = vb[i0 * 3 + 2];
          const float ux = vb[i1 * 3] - ax, uy = vb[i1 * 3 + 1] - ay, uz = vb[i1 * 3 + 2] - az;
          const float vx = vb[i2 * 3] - ax, vy = vb[i2 * 3 + 1] - ay, vz = vb[i2 * 3 + 2] - az;
          const float cx = vw_diff_of_products(uy, vz, uz, vy);
          const float cy = vw_diff_of_products(uz, vx, ux, vz);
          const float cz = vw_diff_of_products(ux, vy, uy, vx);
          const float m = fmaxf(fabsf(cx), fmaxf(fabsf(cy), fabsf(cz)));
          if (m > 0.f) {
            const float sx = cx / m, sy = cy / m, sz = cz / m;
            const float inv = 1.f / sqrtf(sx * sx + sy * sy + sz * sz);
            const float sg = sz > 0.f ? -inv : inv;
            nx = sx * sg; ny = sy * sg; nz = sz * sg;
          }
        }
        const float shade = p.ambient + (1.f - p.ambient) * fmaxf(0.f, -(nx * p.lx + ny * p.ly + nz * p.lz));
        const float* pal = p.palette + who * 3;
        out = vw_u8(255.f * pal[0] * shade) | vw_u8(255.f * pal[1] * shade) << 8 | vw_u8(255.f * pal[2] * shade) << 16;
      }
      uint8_t* o = p.image + gp * 3;
      o[0] = (uint8_t)(out & 255u); o[1] = (uint8_t)((out >> 8) & 255u); o[2] = (uint8_t)(out >> 16);
    }
  }
  // pixels per person, then the scene's: counted by wave, summed in LDS, one global add per entry and workgroup (integers)
  if (p.coverage) {
    for (int n = 0; n <= p.N; ++n) {
      const int c = __popcll(__ballot(who == n));
      if (lane == 0 && c) atomicAdd(&s_cov[n], c);
    }
    __syncthreads();
    if (tid <= p.N && s_cov[tid] != 0) atomicAdd(&p.coverage[t * (p.N + 1) + tid], s_cov[tid]);
  }
}

extern "C" int mh_view_resolve(int T, int N, int V, int F, int H, int W, const uint64_t* keys, const float* verts_view,
                               const int32_t* faces, const uint8_t* point_rgb, const float* palette, const float* light,
                               float ambient, const uint8_t* background, uint8_t* image, float* depth, int32_t* label, int32_t* face,
                               int32_t* coverage, void* stream) {
  MH_CHECK(image || depth || label || face || coverage, "no output requested (every output pointer is null)");
  MH_CHECK(T > 0 && N > 0 && V > 0 && F > 0 && H > 0 && W > 0, "empty input");
  MH_CHECK(N <= VW_MAXN, "more than 32 people per frame");
  MH_CHECK(T <= 65535, "more than 65535 frames in one call (frames are the grid's second dimension)");
  MH_CHECK(H <= VW_MAXDIM && W <= VW_MAXDIM, "image larger than 4096 x 4096");
  MH_CHECK((long long)N * F < 0x80000000ll, "N F must be below 2^31 (person and face share the key's low word with the points)");
  MH_CHECK(keys, "null argument: keys");
  MH_CHECK(!image || (verts_view && faces && palette && light && background),
           "null argument: the image needs the view-space vertices, the faces, a palette, a light direction and a background");
  ViewResolveP p;
  p.T = T; p.N = N; p.V = V; p.F = F; p.H = H; p.W = W;
  p.keys = (const unsigned long long*)keys;
  p.verts = verts_view; p.faces = faces; p.point_rgb = point_rgb; p.palette = palette;
  p.lx = light ? light[0] : 0.f; p.ly = light ? light[1] : 0.f; p.lz = light ? light[2] : 1.f;
  p.ambient = ambient;
  p.bg = background ? ((unsigned)background[0] | (unsigned)background[1] << 8 | (unsigned)background[2] << 16) : 0xffffffu;
  p.image = image; p.depth = depth; p.label = label; p.face = face; p.coverage = coverage;
  hipStream_t st = (hipStream_t)stream;
  if (coverage) MH_HIP(hipMemsetAsync(coverage, 0, (size_t)T * (N + 1) * sizeof(int32_t), st));
  hipLaunchKernelGGL(k_view_resolve, dim3((unsigned)((H * W + VW_BLOCK - 1) / VW_BLOCK), (unsigned)T), dim3(VW_BLOCK), 0, st, p);
  MH_LAUNCH_CHECK();
  return MH_OK;
}
