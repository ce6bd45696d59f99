// Depth ordering between the people of a frame (mh_order_term_keys / mh_order_term, include/mhmocap_hip.h): where the
// instance masks say "this pixel is person y, and certainly not person n", body y must be in front of body n.  The
// image-space coupling of two bodies (Jiang et al., CVPR 2020: the depth-ordering loss), read off the nearest-face keys
// the rasteriser's selection pass has already left for every body separately -- slot 0 of the key records, as
// mh_scene_composite reads them.
//
// One lane per pixel, frames across the grid's y.  Streaming: a lane reads its twice-eroded mask word (4 B); a workgroup
// without any owner ends there, and only a pixel somebody owns goes on to the raw word and to slot 0 of the <= N windows
// that hold it (batched four at a time).  The
// N windows of the frame are decided once per workgroup, by its first N lanes, and kept in LDS; a lane keeps the depths
// of its pixel in an LDS column of its own, so that owners and occluders are walked by bit scans without indexed
// registers.  Sums are 64-bit fixed point (2^-24): integer atomics in LDS, one integer atomic per workgroup and
// accumulator in device memory -- exact in any order, the same bits on every launch.  A tail of one lane per body
// rounds them to float32 once.
//
// The arithmetic is written in the order the header states and compiled without contraction: a float32 evaluation of
// the same expressions on the host gives the same roundings (tests/order_ref.py).
#include "mh_common.h"

#pragma clang fp contract(off)

#define OR_BLOCK 256
#define OR_MAXN 32
#define OR_EMPTY 0xffffffffffffffffull
#define OR_FIX 16777216.0             // 2^24 steps per metre (G) and per square metre (R)
#define OR_RMAX 1024.f
#define OR_ACC 3                      // accumulators per body: G, R, C

struct OrderP {
  int T, N, F, H, W;
  const int* win;                     // [T*N][4] x0, y0, width, height
  const long long* koff;              // [T*N] first window pixel of a body in keys
  const unsigned long long* keys;     // [T*N*H*W][5]
  const unsigned* bits;
  const unsigned* ebits;
  const float* gate;
  float margin, delta;
  long long* acc;                     // [T*N][OR_ACC]
  int* pairs;                         // [T][N][N] or NULL
};

__global__ __launch_bounds__(OR_BLOCK) void k_order_pixels(OrderP p) {
  extern __shared__ float s_z[];                     // [N][OR_BLOCK]: lane tid owns column tid
  __shared__ int s_x0[OR_MAXN], s_y0[OR_MAXN], s_ww[OR_MAXN], s_wh[OR_MAXN];
  __shared__ long long s_ko[OR_MAXN];
  __shared__ unsigned s_live;
  __shared__ unsigned long long s_G[OR_MAXN], s_R[OR_MAXN];
  __shared__ int s_C[OR_MAXN];
  __shared__ int s_pairs[OR_MAXN * OR_MAXN];
  const int tid = threadIdx.x;
  const int t = blockIdx.y, N = p.N, P = p.H * p.W;
  const int i = blockIdx.x * OR_BLOCK + tid;
  const bool inside = i < P;
  const size_t gp = (size_t)t * P + (inside ? i : 0);
  // issued in front of the table loads below: a workgroup then waits for one round trip to memory, not for two in a row
  // (its life is little else: most pixels have no owner)
  const unsigned eword = inside ? p.ebits[gp] : 0u;
  // a workgroup none of whose pixels has an owner among the N people (background: most of them) ends here, before any table
  // is read (uniform: every lane takes part in the vote)
  if (!__syncthreads_or((int)((N >= 32 ? eword : (eword & ((1u << N) - 1u))) != 0u))) return;

  // ---- the frame's bodies: window, first key and whether the body takes part (the whole first wave: one ballot) ------------
  if (tid < 64) {
    bool on = false;
    int x0 = 0, y0 = 0, ww = 0, wh = 0;
    long long ko = 0;
    if (tid < N) {
      const int b = t * N + tid;
      x0 = p.win[b * 4]; y0 = p.win[b * 4 + 1]; ww = p.win[b * 4 + 2]; wh = p.win[b * 4 + 3];
      ko = p.koff[b];
      const long long kcap = (long long)p.T * N * P;
      // as k_scene_composite: a window the selection pass wrote lies inside the image and its keys inside the key array
      on = ww > 0 && wh > 0 && x0 >= 0 && y0 >= 0 && x0 <= p.W - ww && y0 <= p.H - wh && ko >= 0 && ko <= kcap - (long long)ww * wh;
      if (on && p.gate) on = p.gate[b] != 0.f;
    }
    if (tid < OR_MAXN) {
      s_x0[tid] = x0; s_y0[tid] = y0; s_ww[tid] = on ? ww : 0; s_wh[tid] = on ? wh : 0; s_ko[tid] = ko;
      s_G[tid] = 0ull; s_R[tid] = 0ull; s_C[tid] = 0;
    }
    const unsigned long long m = __ballot(on);
    if (tid == 0) s_live = (unsigned)m;
  }
  if (p.pairs)
    for (int k = tid; k < N * N; k += OR_BLOCK) s_pairs[k] = 0;
  __syncthreads();

  unsigned own = eword & s_live;
  if (own) {
    const unsigned raw = p.bits[gp];
    const int y = i / p.W, x = i - y * p.W;
    // ---- z of every body at this pixel: slot 0 of the windows that hold it ---------------------------------------------------
    unsigned def = 0u;
    for (int n0 = 0; n0 < N; n0 += 4) {
      unsigned long long k[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {    // the four loads are in flight together
        const int n = n0 + u;
        k[u] = OR_EMPTY;
        if (n < N) {
          const int x0 = s_x0[n], y0 = s_y0[n], ww = s_ww[n], wh = s_wh[n];
          if (x >= x0 && x < x0 + ww && y >= y0 && y < y0 + wh)
            k[u] = p.keys[((size_t)s_ko[n] + (size_t)(y - y0) * ww + (x - x0)) * 5];
        }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const float z = __uint_as_float((unsigned)(k[u] >> 32));
        const unsigned f = (unsigned)k[u];
        if (k[u] != OR_EMPTY && f < (unsigned)p.F && z > 0.f && z < __builtin_inff()) {     // (false for NaN)
          def |= 1u << (n0 + u);
          s_z[(n0 + u) * OR_BLOCK + tid] = z;
        }
      }
    }
    own &= def;
    const unsigned absent = def & ~raw;
    // ---- owners by bit scan; per owner the bodies the masks rule out here ----------------------------------------------------
    for (unsigned m = own; m; m &= m - 1u) {
      const int yo = __ffs(m) - 1;
      const float zy = s_z[yo * OR_BLOCK + tid];
      long long sm = 0, sr = 0;
      int c = 0;
      for (unsigned o = absent & ~(1u << yo); o; o &= o - 1u) {
        const int n = __ffs(o) - 1;
        const float zn = s_z[n * OR_BLOCK + tid];
        const float d = (zy - zn) + p.margin;
        if (d > 0.f) {
          const float mm = fminf(d, p.delta);
          float r = mm * ((d + d) - mm);
          r = fminf(r, OR_RMAX);
          const long long qm = __double2ll_rn((double)mm * OR_FIX);
          sm += qm;
          sr += __double2ll_rn((double)r * OR_FIX);
          ++c;
          atomicAdd(&s_G[n], (unsigned long long)(-qm));
          if (p.pairs) atomicAdd(&s_pairs[yo * N + n], 1);
        }
      }
      if (c) {
        atomicAdd(&s_G[yo], (unsigned long long)sm);
        atomicAdd(&s_R[yo], (unsigned long long)sr);
        atomicAdd(&s_C[yo], c);
      }
    }
  }
  __syncthreads();
  if (tid < N) {
    unsigned long long* a = (unsigned long long*)p.acc + ((size_t)t * N + tid) * OR_ACC;
    if (s_G[tid] != 0ull) atomicAdd(a, s_G[tid]);
    if (s_R[tid] != 0ull) atomicAdd(a + 1, s_R[tid]);
    if (s_C[tid] != 0) atomicAdd(a + 2, (unsigned long long)s_C[tid]);
  }
  if (p.pairs)
    for (int k = tid; k < N * N; k += OR_BLOCK)
      if (s_pairs[k] != 0) atomicAdd(&p.pairs[(size_t)t * N * N + k], s_pairs[k]);
}

// one lane per body: the sums rounded to float32 once
__global__ void k_order_tail(const long long* acc, int B, int N, float cl, float cg, float* gtransl, float* body_loss, int* count) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const long long G = acc[(size_t)b * OR_ACC], R = acc[(size_t)b * OR_ACC + 1], C = acc[(size_t)b * OR_ACC + 2];
  if (body_loss) body_loss[b] = cl * (float)((double)R * (1.0 / OR_FIX));
  if (count) count[b] = (int)C;
  if (gtransl && N > 1) {             // (one person: nothing can be active, the gradient is not touched)
    const float g = cg * (float)((double)G * (1.0 / OR_FIX));
    gtransl[(size_t)b * 3 + 2] += g;
  }
}

// every check that needs no table
static int order_check(int T, int N, int F, int H, int W, float margin, float delta, bool any_output) {
  MH_CHECK(any_output, "no output requested (gtransl, body_loss, count and pairs are all null)");
  MH_CHECK(T > 0 && N > 0 && F > 0 && H > 0 && W > 0, "empty input");
  MH_CHECK(N <= OR_MAXN, "more than 32 people per frame");
  MH_CHECK(margin >= 0.f, "margin must not be negative");
  MH_CHECK(delta > 0.f && delta <= OR_RMAX, "delta must lie in (0, 1024]");
  MH_CHECK((long long)N * H * W <= (1ll << 26), "N H W above 2^26: the 64-bit fixed-point sums of a body (2^-24 steps, terms up to 1024) "
                                               "are only known to stay below 2^61 up to there");
  MH_CHECK(T <= 65535, "more than 65535 frames in one call (frames are the grid's second dimension)");
  MH_CHECK(H <= 4095 && W <= 65535, "image larger than the rasteriser's windows can be (4095 rows, 65535 columns)");
  return MH_OK;
}

extern "C" int mh_order_term_keys(int T, int N, int F, int H, int W, const int32_t* win, const int64_t* koff, const uint64_t* keys,
                                  const uint32_t* bits, const uint32_t* ebits, const float* gate, float coef, float margin,
                                  float delta, float* gtransl, float* body_loss, int32_t* count, int32_t* pairs, void* acc,
                                  void* stream) {
  if (int rc = order_check(T, N, F, H, W, margin, delta, gtransl || body_loss || count || pairs)) return rc;
  MH_CHECK(win && koff && keys, "null argument: win, koff and keys");
  MH_CHECK(bits && ebits, "null argument: bits and ebits");
  hipStream_t st = (hipStream_t)stream;
  const size_t TN = (size_t)T * N, acc_bytes = TN * OR_ACC * sizeof(long long);
  OrderP p;
  p.T = T; p.N = N; p.F = F; p.H = H; p.W = W;
  p.win = (const int*)win; p.koff = (const long long*)koff; p.keys = (const unsigned long long*)keys;
  p.bits = (const unsigned*)bits; p.ebits = (const unsigned*)ebits; p.gate = gate;
  p.margin = margin; p.delta = delta;
  p.acc = (long long*)acc;
  p.pairs = (int*)pairs;
  bool own = false, pooled = true;
  if (!p.acc) {
    // as mh_scene_pen_term: from the stream's memory pool, back to it behind the two kernels
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cs) != hipSuccess) (void)hipGetLastError();
    MH_CHECK(cs == hipStreamCaptureStatusNone, "the stream is capturing: the accumulators must come from the caller (acc, 24 bytes per body)");
    own = true;
    if (hipMallocAsync((void**)&p.acc, acc_bytes, st) != hipSuccess) {
      (void)hipGetLastError();
      p.acc = nullptr;
      pooled = false;
      MH_HIP(hipMalloc((void**)&p.acc, acc_bytes));
    }
  }
  hipError_t e = hipMemsetAsync(p.acc, 0, acc_bytes, st);
  if (e == hipSuccess && pairs) e = hipMemsetAsync(pairs, 0, TN * N * sizeof(int32_t), st);
  if (e != hipSuccess) {
    if (own && pooled) (void)hipFreeAsync(p.acc, st);
    if (own && !pooled) (void)hipFree(p.acc);
    mh_set_error("hipMemsetAsync failed: %s (%s:%d)", hipGetErrorString(e), __FILE__, __LINE__);
    return MH_ERR_HIP;
  }
  const int P = H * W;
  hipLaunchKernelGGL(k_order_pixels, dim3((unsigned)((P + OR_BLOCK - 1) / OR_BLOCK), (unsigned)T), dim3(OR_BLOCK),
                     (size_t)N * OR_BLOCK * sizeof(float), st, p);
  hipError_t le = hipGetLastError();
  if (le == hipSuccess && (gtransl || body_loss || count)) {
    const float cl = (float)((double)coef / (double)P), cg = (float)(2.0 * (double)coef / (double)P);
    hipLaunchKernelGGL(k_order_tail, dim3((unsigned)((TN + 255) / 256)), dim3(256), 0, st, p.acc, (int)TN, N, cl, cg, gtransl,
                       body_loss, count);
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

extern "C" int mh_order_term(int T, int N, int V, int F, int H, int W, const void* ws, const uint32_t* bits, const uint32_t* ebits,
                             const float* gate, float coef, float margin, float delta, float* gtransl, float* body_loss,
                             int32_t* count, int32_t* pairs, void* acc, void* stream) {
  MH_CHECK(ws, "null argument: ws");
  size_t off[3];                      // (refuses empty dimensions, V among them; everything else is the callee's to check)
  if (int rc = mh_raster_workspace_offsets(T, N, V, F, H, W, off)) return rc;
  const char* w = (const char*)ws;
  return mh_order_term_keys(T, N, F, H, W, (const int32_t*)(w + off[0]), (const int64_t*)(w + off[1]), (const uint64_t*)(w + off[2]),
                            bits, ebits, gate, coef, margin, delta, gtransl, body_loss, count, pairs, acc, stream);
}
