// Scene composite over the people of a frame (mh_scene_composite, include/mhmocap_hip.h): from the nearest-face keys a
// selection pass of the rasteriser left in its workspace -- one window per body, slot 0 of every window pixel's key record
// = float bits of z << 32 | face -- to images of the fitted scene: who owns a pixel and with which face, metric depth,
// geometric normals, a shaded overlay on the input frame, pixel-sampled vertex visibility and per-person pixel counts.
// Replaces the reference's matplotlib scatter plots of projected vertices (predict.py:195-243).
//
// One lane per pixel, frames across the grid's y.  Streaming: a lane reads the 8-byte slot 0 of the <= N windows that
// contain its pixel (the records are 40 bytes apart: every cache line of a covered window row is touched) and writes
// depth + person + face + normal + overlay = 27 bytes; the gathers behind a covered pixel (3 indices, 9 coordinates of
// the winning face) hit a body's 80 KB of vertices in L2.
#include "mh_common.h"

#define RC_BLOCK 256
#define RC_MAXN 32
#define RC_EMPTY 0xffffffffffffffffull

struct CompositeP {
  int T, N, V, F, H, W;
  const float* verts;
  const int* faces;
  const int* win;                     // [T*N][4] x0, y0, width, height
  const long long* koff;              // [T*N] first window pixel of a body in keys
  const unsigned long long* keys;     // [T*N*H*W][5]
  const uint8_t* images;
  const float* palette;
  float lx, ly, lz, ambient, alpha;
  float* depth;
  int* person;
  int* face;
  float* normal;
  uint8_t* overlay;
  uint8_t* visible;
  int* coverage;
  int packed;                         // overlay (and images) are moved as 3 dwords per 4 pixels
};

// a b - c d, the product c d compensated (Kahan): a cross product of two short edges cancels, and a plain fp32
// evaluation loses its leading digits there
__device__ __forceinline__ float rc_diff_of_products(float a, float b, float c, float d) {
  const float w = c * d;
  const float e = fmaf(-c, d, w);
  const float f = fmaf(a, b, -w);
  return f + e;
}

__device__ __forceinline__ unsigned rc_u8(float v) {
  return (unsigned)__float2int_rn(fminf(fmaxf(v, 0.f), 255.f));
}

__global__ __launch_bounds__(RC_BLOCK) void k_scene_composite(CompositeP p) {
  __shared__ int s_cov[RC_MAXN];
  const int tid = threadIdx.x, lane = tid & 63;      // (a workgroup is whole waves: every lane takes part in the shuffles and ballots below)
  const int t = blockIdx.y, P = p.H * p.W;
  const int i = blockIdx.x * RC_BLOCK + tid;
  const bool inside = i < P;
  const int y = inside ? i / p.W : 0, x = inside ? i - y * p.W : 0;
  if (p.coverage && tid < RC_MAXN) s_cov[tid] = 0;
  if (p.coverage) __syncthreads();

  // ---- winner over the bodies whose window holds the pixel: smallest (z, n) ------------------------------------------------
  float best_z = 0.f;
  int best_n = -1, best_f = -1;
  const long long kcap = (long long)p.T * p.N * P;
  for (int n0 = 0; n0 < p.N; n0 += 4) {
    unsigned long long k[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {      // the four loads are in flight together
      const int n = n0 + u;
      k[u] = RC_EMPTY;
      if (n < p.N) {
        const int b = t * p.N + n;
        const int x0 = p.win[b * 4], y0 = p.win[b * 4 + 1], ww = p.win[b * 4 + 2], wh = p.win[b * 4 + 3];
        const long long ko = p.koff[b];
        // a window the selection pass wrote lies inside the image and its keys inside the key array; anything else
        // (a body with nothing on screen: width <= 0) is skipped
        const bool ok = ww > 0 && wh > 0 && x0 >= 0 && y0 >= 0 && x0 <= p.W - ww && y0 <= p.H - wh && ko >= 0 &&
                        ko <= kcap - (long long)ww * wh;
        if (ok && inside && x >= x0 && x < x0 + ww && y >= y0 && y < y0 + wh)
          k[u] = p.keys[((size_t)ko + (size_t)(y - y0) * ww + (x - x0)) * 5];
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const float z = __uint_as_float((unsigned)(k[u] >> 32));
      const unsigned f = (unsigned)k[u];
      if (k[u] != RC_EMPTY && f < (unsigned)p.F && (best_n < 0 || z < best_z)) { best_z = z; best_n = n0 + u; best_f = (int)f; }
    }
  }
  const size_t gp = (size_t)t * P + i;
  if (inside) {
    if (p.depth) p.depth[gp] = best_n >= 0 ? best_z : -1.f;
    if (p.person) p.person[gp] = best_n;
    if (p.face) p.face[gp] = best_f;
  }

  // ---- the winning face: visibility of its vertices, geometric normal towards the camera ------------------------------------
  float nx = 0.f, ny = 0.f, nz = 0.f;
  if (best_n >= 0 && (p.normal || p.overlay || p.visible)) {
    const int b = t * p.N + best_n;
    const int i0 = p.faces[best_f * 3], i1 = p.faces[best_f * 3 + 1], i2 = p.faces[best_f * 3 + 2];
    if ((unsigned)i0 < (unsigned)p.V && (unsigned)i1 < (unsigned)p.V && (unsigned)i2 < (unsigned)p.V) {
      if (p.visible) {                 // plain stores of the constant 1: idempotent, no atomics
        uint8_t* vis = p.visible + (size_t)b * p.V;
        vis[i0] = 1; vis[i1] = 1; vis[i2] = 1;
      }
      if (p.normal || p.overlay) {
        const float* vb = p.verts + (size_t)b * p.V * 3;
        const float ax = vb[i0 * 3], ay = vb[i0 * 3 + 1], az = vb[i0 * 3 + 2];
        const float ux = vb[i1 * 3] - ax, uy = vb[i1 * 3 + 1] - ay, uz = vb[i1 * 3 + 2] - az;
        const float vx = vb[i2 * 3] - ax, vy = vb[i2 * 3 + 1] - ay, vz = vb[i2 * 3 + 2] - az;
        const float cx = rc_diff_of_products(uy, vz, uz, vy);
        const float cy = rc_diff_of_products(uz, vx, ux, vz);
        const float cz = rc_diff_of_products(ux, vy, uy, vx);
        // scaled by the largest component first: the squares of a sliver's cross product must not underflow
        const float m = fmaxf(fabsf(cx), fmaxf(fabsf(cy), fabsf(cz)));
        if (m > 0.f) {
          const float sx = cx / m, sy = cy / m, sz = cz / m;
          const float inv = 1.f / sqrtf(sx * sx + sy * sy + sz * sz);
          const float sg = sz > 0.f ? -inv : inv;
          nx = sx * sg; ny = sy * sg; nz = sz * sg;
        }
      }
    }
  }
  if (inside && p.normal) {
    float* o = p.normal + gp * 3;
    o[0] = nx; o[1] = ny; o[2] = nz;
  }

  // ---- overlay: the person's colour, shaded, blended over the frame --------------------------------------------------------
  if (p.overlay) {
    // pixel as r | g << 8 | b << 16.  packed: the 12 bytes of 4 neighbouring pixels are 3 aligned dwords; lane j < 3 of
    // the four moves dword j and the bytes change lanes by shuffles (every lane of the wave gets here)
    const int quad = lane & ~3, j = lane & 3;
    const size_t qbyte = (gp - j) * 3 + (size_t)j * 4;       // dword j of the four pixels
    unsigned img = 0u;
    if (p.images) {
      if (p.packed) {
        unsigned d = 0u;
        if (inside && j < 3) d = *(const unsigned*)(p.images + qbyte);
        const int lo = (3 * j) >> 2, hi = min(lo + 1, 2);
        const unsigned dlo = __shfl(d, quad + lo, 64), dhi = __shfl(d, quad + hi, 64);
        img = (unsigned)((((unsigned long long)dhi << 32) | dlo) >> (8 * ((3 * j) & 3))) & 0xffffffu;
      } else if (inside) {
        const uint8_t* s = p.images + gp * 3;
        img = (unsigned)s[0] | (unsigned)s[1] << 8 | (unsigned)s[2] << 16;
      }
    }
    unsigned out = img;
    if (best_n >= 0) {
      const float shade = p.ambient + (1.f - p.ambient) * fmaxf(0.f, -(nx * p.lx + ny * p.ly + nz * p.lz));
      const float* pal = p.palette + best_n * 3;
      const float ia = 1.f - p.alpha;
      const unsigned r = rc_u8(ia * (float)(img & 255u) + p.alpha * (255.f * pal[0] * shade));
      const unsigned g = rc_u8(ia * (float)((img >> 8) & 255u) + p.alpha * (255.f * pal[1] * shade));
      const unsigned bl = rc_u8(ia * (float)((img >> 16) & 255u) + p.alpha * (255.f * pal[2] * shade));
      out = r | g << 8 | bl << 16;
    }
    if (p.packed) {
      const int pa = min((4 * j) / 3, 3), pb = min(pa + 1, 3);
      const unsigned a = __shfl(out, quad + pa, 64), b2 = __shfl(out, quad + pb, 64);
      const unsigned d = (unsigned)(((unsigned long long)a | ((unsigned long long)b2 << 24)) >> (8 * ((4 * j) % 3)));
      if (inside && j < 3) *(unsigned*)(p.overlay + qbyte) = d;
    } else if (inside) {
      uint8_t* o = p.overlay + gp * 3;
      o[0] = (uint8_t)(out & 255u); o[1] = (uint8_t)((out >> 8) & 255u); o[2] = (uint8_t)(out >> 16);
    }
  }

  // ---- pixels per person: counted by wave, summed in LDS, one global add per person and workgroup (integers: exact in any order)
  if (p.coverage) {
    for (int n = 0; n < p.N; ++n) {
      const int c = __popcll(__ballot(best_n == n));
      if (lane == 0 && c) atomicAdd(&s_cov[n], c);
    }
    __syncthreads();
    if (tid < p.N && s_cov[tid] != 0) atomicAdd(&p.coverage[t * p.N + tid], s_cov[tid]);
  }
}

extern "C" int mh_scene_composite(int T, int N, int V, int F, int H, int W, const float* verts, const int32_t* faces,
                                  const void* ws, const uint8_t* images, const float* palette, const float* light,
                                  float ambient, float alpha, float* depth, int32_t* person, int32_t* face, float* normal,
                                  uint8_t* overlay, uint8_t* visible, int32_t* coverage, void* stream) {
  MH_CHECK(depth || person || face || normal || overlay || visible || coverage, "no output requested (every output pointer is null)");
  MH_CHECK(T > 0 && N > 0 && V > 0 && F > 0 && H > 0 && W > 0, "empty input");
  MH_CHECK(N <= RC_MAXN, "more than 32 people per frame");
  MH_CHECK(T <= 65535, "more than 65535 frames in one call (frames are the grid's second dimension)");
  MH_CHECK(H <= 4095 && W <= 65535, "image larger than the rasteriser's windows can be (4095 rows, 65535 columns)");
  MH_CHECK(ws && faces, "null argument");
  MH_CHECK(verts || !(normal || overlay), "null argument: normals and the overlay's shading read the vertices");
  MH_CHECK(!overlay || (palette && light), "null argument: the overlay needs a palette and a light direction");
  size_t off[3];
  if (int rc = mh_raster_workspace_offsets(T, N, V, F, H, W, off)) return rc;
  CompositeP p;
  p.T = T; p.N = N; p.V = V; p.F = F; p.H = H; p.W = W;
  p.verts = verts; p.faces = faces;
  p.win = (const int*)((const char*)ws + off[0]);
  p.koff = (const long long*)((const char*)ws + off[1]);
  p.keys = (const unsigned long long*)((const char*)ws + off[2]);
  p.images = images; p.palette = palette;
  p.lx = light ? light[0] : 0.f; p.ly = light ? light[1] : 0.f; p.lz = light ? light[2] : -1.f;
  p.ambient = ambient; p.alpha = alpha;
  p.depth = depth; p.person = person; p.face = face; p.normal = normal;
  p.overlay = overlay; p.visible = visible; p.coverage = coverage;
  // 4 pixels = 3 dwords: whole groups of four, dword-aligned in every frame
  p.packed = ((H * W) % 4 == 0 && ((uintptr_t)overlay & 3) == 0 && ((uintptr_t)images & 3) == 0) ? 1 : 0;
  hipStream_t st = (hipStream_t)stream;
  if (coverage) MH_HIP(hipMemsetAsync(coverage, 0, (size_t)T * N * sizeof(int32_t), st));
  hipLaunchKernelGGL(k_scene_composite, dim3((H * W + RC_BLOCK - 1) / RC_BLOCK, T), dim3(RC_BLOCK), 0, st, p);
  MH_LAUNCH_CHECK();
  return MH_OK;
}
