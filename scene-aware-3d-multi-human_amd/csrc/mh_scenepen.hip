// Scene penetration with gradients (mh_scene_zmap / mh_scene_pen_term / mh_scene_pen_term_sel, include/mhmocap_hip.h):
// every vertex of every body against the scene's depth map, bilinearly interpolated, so that the gradient of a vertex
// on a planar piece of the scene is parallel to that plane's normal (behind the surface it tilts towards the optical
// axis by (p + margin) / z: the header has the exact form).  The backward half of mh_fit_report_verts.
//
// One lane per vertex of the flat (B*V) list: 12 B read per vertex, four taps of the map (a few hundred KB: cache
// resident), 12 B of gradient loaded and 12 B stored for the active vertices only.  A vertex is owned by one lane, so
// the gradient is a plain load, add and store.  The per-body sum of p^2 is carried as 64-bit fixed point -- integer LDS
// atomics, one integer device atomic per workgroup and body, rounded to float32 once -- and has the same bits on every
// launch.
//
// The arithmetic is written in the order the header states and compiled without contraction: a float32 evaluation of
// the same expressions on the host gives the same roundings (tests/scene_pen_ref.py).
#include "mh_common.h"

#pragma clang fp contract(off)

#define SP_BLOCK 256
#define SP_FIX 1099511627776.0        // 2^40 steps per square metre
#define SP_SUM_MAX 8388608.0          // band^2 V below 2^23 m^2: the sum of a body stays below 2^63 steps

struct ScenePenP {
  int n, V, H, W;                     // n = B V vertices
  float fx, fy, cx, cy;
  float coef, margin, band, edge;
  const float* verts;
  const float* zmap0;
  const float* zmap1;
  const int* words;                   // [scene live, which map] (mh_scene_pen_term_sel) or NULL: zmap0
  float* gverts;
  unsigned long long* acc;            // [B] fixed-point sums of p^2, or NULL
};

__global__ __launch_bounds__(SP_BLOCK) void k_scene_pen(ScenePenP p) {
  __shared__ unsigned long long s_sum[SP_BLOCK];      // one slot per body this workgroup can touch (V >= 1)
  const int tid = threadIdx.x;
  const float* zmap = p.zmap0;
  if (p.words) {
    if (p.words[0] == 0) return;                      // no scene yet: nothing is read or written (the sums stay 0)
    if (p.words[1] != 0) zmap = p.zmap1;
  }
  const int i0 = blockIdx.x * SP_BLOCK, i = i0 + tid;
  const int b0 = i0 / p.V;
  const bool sums = p.acc != nullptr;
  if (sums) s_sum[tid] = 0ull;
  __syncthreads();
  if (i < p.n) {
    const int b = i / p.V;
    const float* q = p.verts + (size_t)i * 3;
    const float x = q[0], y = q[1], z = q[2];
    if (z > 0.f) {
      const float u = p.fx * x / z + p.cx, v = p.fy * y / z + p.cy;
      const float uc = u - 0.5f, vc = v - 0.5f;
      const float fi = floorf(uc), fj = floorf(vc);
      // all four taps inside the image (false for NaN)
      if (fi >= 0.f && fi + 1.f <= (float)(p.W - 1) && fj >= 0.f && fj + 1.f <= (float)(p.H - 1)) {
        const float a = uc - fi, bb = vc - fj;
        const float* r0 = zmap + (size_t)(int)fj * p.W + (int)fi;
        const float* r1 = r0 + p.W;
        const float D00 = r0[0], D10 = r0[1], D01 = r1[0], D11 = r1[1];
        const float lo = fminf(fminf(D00, D10), fminf(D01, D11)), hi = fmaxf(fmaxf(D00, D10), fmaxf(D01, D11));
        if (D00 > 0.f && D10 > 0.f && D01 > 0.f && D11 > 0.f && hi - lo <= p.edge) {
          const float a1 = 1.f - a, b1 = 1.f - bb;
          const float D = b1 * (a1 * D00 + a * D10) + bb * (a1 * D01 + a * D11);
          const float pen = z - D - p.margin;
          if (pen > 0.f && pen < p.band) {
            if (sums) {
              const double pd = (double)pen;
              atomicAdd(&s_sum[b - b0], (unsigned long long)__double2ll_rn(pd * pd * SP_FIX));
            }
            if (p.gverts) {
              const float Du = b1 * (D10 - D00) + bb * (D11 - D01);
              const float Dv = a1 * (D01 - D00) + a * (D11 - D10);
              const float g = 2.f * p.coef * pen / (float)p.V;
              float* o = p.gverts + (size_t)i * 3;
              o[0] += -(g * Du * p.fx / z);
              o[1] += -(g * Dv * p.fy / z);
              o[2] += g * (1.f + (Du * p.fx * x + Dv * p.fy * y) / (z * z));
            }
          }
        }
      }
    }
  }
  if (!sums) return;                                  // (uniform)
  __syncthreads();
  const int last = min(p.n, i0 + SP_BLOCK) - 1;
  if (tid <= last / p.V - b0 && s_sum[tid] != 0ull) atomicAdd(&p.acc[b0 + tid], s_sum[tid]);
}

__global__ void k_scene_pen_sums(const unsigned long long* acc, float* body_loss, int B, double scale) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b < B) body_loss[b] = (float)((double)acc[b] * scale);
}

__global__ void k_scene_zmap(const float* depth, const float* mask, float* zmap, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) zmap[i] = mask[i] > 0.5f ? depth[i] : 0.f;
}

extern "C" int mh_scene_zmap(int H, int W, const float* depth, const float* mask, float* zmap, void* stream) {
  MH_CHECK(H > 0 && W > 0, "empty input");
  MH_CHECK((long long)H * W <= 0x7fffffffll - 256, "image too large");
  MH_CHECK(depth && mask && zmap, "null argument");
  const int n = H * W;
  hipLaunchKernelGGL(k_scene_zmap, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, depth, mask, zmap, n);
  MH_LAUNCH_CHECK();
  return MH_OK;
}

static int scene_pen_launch(int B, int V, int H, int W, const float* K, const float* verts, const float* zmap0, const float* zmap1,
                            const int32_t* words, float coef, float margin, float band, float edge, float* gverts,
                            float* body_loss, void* acc_ws, void* stream) {
  MH_CHECK(B > 0 && V > 0 && H > 0 && W > 0, "empty input");
  MH_CHECK((long long)H * W <= 0x7fffffffll && H <= (1 << 24) && W <= (1 << 24), "image too large");
  MH_CHECK((long long)B * V <= 0x7fffffffll - SP_BLOCK, "too many vertices for one launch");
  MH_CHECK(K && verts, "null argument: K and verts");
  MH_CHECK(zmap0 && (zmap1 || !words), "null argument: zmap");
  MH_CHECK(margin >= 0.f, "margin must not be negative");
  MH_CHECK(band > 0.f, "band must be positive");
  MH_CHECK(edge > 0.f, "edge must be positive");
  MH_CHECK((double)band * band * V < SP_SUM_MAX, "band^2 V too large for the fixed-point sum of a body");
  hipStream_t st = (hipStream_t)stream;
  ScenePenP p;
  p.n = B * V; p.V = V; p.H = H; p.W = W;
  p.fx = K[0]; p.cx = K[2]; p.fy = K[4]; p.cy = K[5];
  p.coef = coef; p.margin = margin; p.band = band; p.edge = edge;
  p.verts = verts; p.zmap0 = zmap0; p.zmap1 = zmap1; p.words = (const int*)words;
  p.gverts = gverts;
  p.acc = nullptr;
  bool own = false, pooled = true;
  if (body_loss) {
    p.acc = (unsigned long long*)acc_ws;
    if (!p.acc) {
      // as mh_fit_report_pixels: from the stream's memory pool, back to it behind the two kernels
      hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
      if (hipStreamIsCapturing(st, &cs) != hipSuccess) (void)hipGetLastError();
      MH_CHECK(cs == hipStreamCaptureStatusNone, "the stream is capturing: the accumulators must come from the caller (acc, 8 bytes per body)");
      own = true;
      if (hipMallocAsync((void**)&p.acc, (size_t)B * 8, st) != hipSuccess) {
        (void)hipGetLastError();
        p.acc = nullptr;
        pooled = false;
        MH_HIP(hipMalloc((void**)&p.acc, (size_t)B * 8));
      }
    }
    hipError_t e = hipMemsetAsync(p.acc, 0, (size_t)B * 8, st);
    if (e != hipSuccess) {
      if (own && pooled) (void)hipFreeAsync(p.acc, st);
      if (own && !pooled) (void)hipFree(p.acc);
      mh_set_error("hipMemsetAsync failed: %s (%s:%d)", hipGetErrorString(e), __FILE__, __LINE__);
      return MH_ERR_HIP;
    }
  }
  hipLaunchKernelGGL(k_scene_pen, dim3((unsigned)((p.n + SP_BLOCK - 1) / SP_BLOCK)), dim3(SP_BLOCK), 0, st, p);
  hipError_t le = hipGetLastError();
  if (le == hipSuccess && p.acc) {
    hipLaunchKernelGGL(k_scene_pen_sums, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, st, p.acc, body_loss, B,
                       (double)coef / ((double)V * SP_FIX));
    le = hipGetLastError();
  }
  if (own && pooled) (void)hipFreeAsync(p.acc, st);           // stream-ordered: behind the two kernels
  if (own && !pooled) { (void)hipStreamSynchronize(st); (void)hipFree(p.acc); }
  if (le != hipSuccess) {
    mh_set_error("kernel launch failed: %s (%s:%d)", hipGetErrorString(le), __FILE__, __LINE__);
    return MH_ERR_HIP;
  }
  return MH_OK;
}

extern "C" int mh_scene_pen_term(int B, int V, int H, int W, const float* K, const float* verts, const float* zmap, float coef,
                                 float margin, float band, float edge, float* gverts, float* body_loss, void* acc, void* stream) {
  return scene_pen_launch(B, V, H, W, K, verts, zmap, nullptr, nullptr, coef, margin, band, edge, gverts, body_loss, acc, stream);
}

extern "C" int mh_scene_pen_term_sel(int B, int V, int H, int W, const float* K, const float* verts, const float* zmap0,
                                     const float* zmap1, const int32_t* words, float coef, float margin, float band, float edge,
                                     float* gverts, float* body_loss, void* acc, void* stream) {
  MH_CHECK(words, "null argument: words");
  return scene_pen_launch(B, V, H, W, K, verts, zmap0, zmap1, words, coef, margin, band, edge, gverts, body_loss, acc, stream);
}
