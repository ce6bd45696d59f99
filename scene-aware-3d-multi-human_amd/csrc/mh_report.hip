// The fit in numbers (mh_fit_report_pixels / mh_fit_report_verts, include/mhmocap_hip.h): per frame and person, how the
// rendered body covers its instance mask, how far its depth is from the target depth, how much of it lies behind the
// scene's surface -- and, per body, how many vertices are inside the scene and how deep.  Read-only on the inputs.
//
// Pixels: a streaming pass at 16 B per pixel (label, depth, mask word, disparity) with outputs of a few bytes per person.
// A lane adds what its pixel contributes into the workgroup's LDS table by INTEGER atomics (a background pixel adds
// nothing); the table goes to device memory by one integer atomic per non-zero entry and workgroup.  The two float sums
// are carried as 64-bit fixed point, so every sum is exact in any order and has the same bits on every launch.
#include "mh_common.h"

#define RP_BLOCK 128
#define RP_MAXN 32
#define RP_UNROLL 4
#define RP_TARGET_BLOCKS 2048
#define RP_FIX 268435456.0            // 2^28 steps per metre
#define RP_CLAMP 1e9f

struct ReportP {
  int T, N, P;
  int ppb, bpf;                       // pixels per workgroup (a multiple of RP_BLOCK), workgroups per frame
  const int* person;
  const float* depth;
  const unsigned* bits;
  const float* disp;
  const float* min_z;
  const float* max_z;
  const float* scene_depth;
  const uint8_t* scene_mask;
  float depth_offset, margin;
  int* counts;
  long long* acc;                     // [T*N][2] fixed-point sums, or NULL
};

__global__ __launch_bounds__(RP_BLOCK) void k_fit_report_pixels(ReportP p) {
  __shared__ int s_cnt[RP_MAXN * 4];
  __shared__ unsigned long long s_sum[RP_MAXN * 2];
  const int tid = threadIdx.x;
  const int t = blockIdx.x / p.bpf, seg = blockIdx.x - t * p.bpf;
  for (int k = tid; k < RP_MAXN * 4; k += RP_BLOCK) s_cnt[k] = 0;
  for (int k = tid; k < RP_MAXN * 2; k += RP_BLOCK) s_sum[k] = 0ull;
  __syncthreads();
  const bool sums = p.acc != nullptr;
  const bool scene = p.scene_depth != nullptr;
  float za = 0.f, zb = 0.f;
  if (sums) {
    zb = 1.f / p.max_z[t];
    za = 1.f / p.min_z[t] - zb;
  }
  const unsigned live = p.N >= 32 ? 0xffffffffu : ((1u << p.N) - 1u);
  const int lo = seg * p.ppb, hi = min(p.P, lo + p.ppb);
  const size_t base = (size_t)t * p.P;
  for (int i0 = lo + tid; i0 < hi; i0 += RP_BLOCK * RP_UNROLL) {
    int who[RP_UNROLL];
    unsigned w[RP_UNROLL];
    float z[RP_UNROLL], dp[RP_UNROLL], sd[RP_UNROLL];
    unsigned sm[RP_UNROLL];
#pragma unroll
    for (int u = 0; u < RP_UNROLL; ++u) {          // the loads of the four pixels are in flight together
      const int i = i0 + u * RP_BLOCK;
      who[u] = -1; w[u] = 0u; z[u] = 0.f; dp[u] = 0.f; sd[u] = 0.f; sm[u] = 0u;
      if (i < hi) {
        who[u] = p.person[base + i];
        w[u] = p.bits[base + i] & live;
        z[u] = p.depth[base + i];
        if (sums) dp[u] = p.disp[base + i];
        if (scene) { sd[u] = p.scene_depth[i]; sm[u] = p.scene_mask[i]; }
      }
    }
#pragma unroll
    for (int u = 0; u < RP_UNROLL; ++u) {
      const int n = who[u];
      const bool drawn = n >= 0 && n < p.N;
      for (unsigned m = w[u]; m; m &= m - 1u) atomicAdd(&s_cnt[(__ffs(m) - 1) * 4 + 1], 1);
      if (!drawn) continue;
      atomicAdd(&s_cnt[n * 4], 1);
      if (scene && sm[u] != 0u) {
        const float surface = sd[u] + p.margin;
        if (z[u] > surface) atomicAdd(&s_cnt[n * 4 + 3], 1);
      }
      if ((w[u] >> n) & 1u) {
        atomicAdd(&s_cnt[n * 4 + 2], 1);
        if (sums) {
          float d = z[u] + p.depth_offset - 1.f / (dp[u] * za + zb);
          d = fminf(fmaxf(d, -RP_CLAMP), RP_CLAMP);
          const long long q = __double2ll_rn((double)d * RP_FIX);
          const long long qa = q < 0 ? -q : q;
          atomicAdd(&s_sum[n * 2], (unsigned long long)q);
          atomicAdd(&s_sum[n * 2 + 1], (unsigned long long)qa);
        }
      }
    }
  }
  __syncthreads();
  if (p.counts)
    for (int k = tid; k < p.N * 4; k += RP_BLOCK)
      if (s_cnt[k] != 0) atomicAdd(&p.counts[(size_t)t * p.N * 4 + k], s_cnt[k]);
  if (sums)
    for (int k = tid; k < p.N * 2; k += RP_BLOCK)
      if (s_sum[k] != 0ull) atomicAdd((unsigned long long*)&p.acc[(size_t)t * p.N * 2 + k], s_sum[k]);
}

__global__ void k_fit_report_sums(const long long* acc, float* dsum, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dsum[i] = (float)((double)acc[i] * (1.0 / RP_FIX));
}

extern "C" int mh_fit_report_pixels(int T, int N, int H, int W, const int32_t* person, const float* depth, const uint32_t* bits,
                                    const float* disp, const float* min_z, const float* max_z, const float* scene_depth,
                                    const uint8_t* scene_mask, float depth_offset, float margin, int32_t* counts, float* dsum,
                                    void* stream) {
  MH_CHECK(counts || dsum, "no output requested (counts and dsum are both null)");
  MH_CHECK(T > 0 && N > 0 && H > 0 && W > 0, "empty input");
  MH_CHECK(N <= RP_MAXN, "more than 32 people per frame");
  MH_CHECK((long long)H * W <= 0x7fffffffll - RP_BLOCK * RP_UNROLL, "image too large (pixels of a frame are indexed by 32 bits)");
  MH_CHECK(person && depth && bits, "null argument: person, depth and bits are read for every pixel");
  MH_CHECK(!disp || (min_z && max_z), "disp given without min_z or max_z");
  MH_CHECK((scene_depth != nullptr) == (scene_mask != nullptr), "only one of scene_depth and scene_mask given");
  hipStream_t st = (hipStream_t)stream;
  const int P = H * W;
  const size_t TN = (size_t)T * N;
  ReportP p;
  p.T = T; p.N = N; p.P = P;
  // about RP_TARGET_BLOCKS workgroups whatever T is: one frame is cut into up to P / RP_BLOCK pieces, 2000 frames into one or two each
  const int per_frame = (P + RP_BLOCK - 1) / RP_BLOCK;
  long long want = (RP_TARGET_BLOCKS + (long long)T - 1) / T;
  want = want < 1 ? 1 : (want > per_frame ? per_frame : want);
  p.ppb = (int)(((P + want - 1) / want + RP_BLOCK - 1) / RP_BLOCK) * RP_BLOCK;
  p.bpf = (P + p.ppb - 1) / p.ppb;
  MH_CHECK((long long)T * p.bpf <= 0x7fffffffll, "too many frames for one launch");
  p.person = person; p.depth = depth; p.bits = bits;
  p.disp = disp; p.min_z = min_z; p.max_z = max_z;
  p.scene_depth = scene_depth; p.scene_mask = scene_mask;
  p.depth_offset = depth_offset; p.margin = margin;
  p.counts = counts;
  p.acc = nullptr;
  bool pooled = true;
  if (counts) MH_HIP(hipMemsetAsync(counts, 0, TN * 4 * sizeof(int32_t), st));
  if (dsum && !disp) MH_HIP(hipMemsetAsync(dsum, 0, TN * 2 * sizeof(float), st));
  if (dsum && disp) {
    if (hipMallocAsync((void**)&p.acc, TN * 2 * sizeof(long long), st) != hipSuccess) {
      // a device without a memory pool: a plain allocation, returned after the stream has drained
      (void)hipGetLastError();
      p.acc = nullptr;
      pooled = false;
      MH_HIP(hipMalloc((void**)&p.acc, TN * 2 * sizeof(long long)));
    }
    hipError_t e = hipMemsetAsync(p.acc, 0, TN * 2 * sizeof(long long), st);
    if (e != hipSuccess) {
      if (pooled) (void)hipFreeAsync(p.acc, st); else (void)hipFree(p.acc);
      mh_set_error("hipMemsetAsync failed: %s (%s:%d)", hipGetErrorString(e), __FILE__, __LINE__);
      return MH_ERR_HIP;
    }
  }
  hipLaunchKernelGGL(k_fit_report_pixels, dim3((unsigned)(T * p.bpf)), dim3(RP_BLOCK), 0, st, p);
  hipError_t le = hipGetLastError();
  if (le == hipSuccess && p.acc) {
    hipLaunchKernelGGL(k_fit_report_sums, dim3((unsigned)((TN * 2 + 255) / 256)), dim3(256), 0, st, p.acc, dsum, TN * 2);
    le = hipGetLastError();
  }
  if (p.acc && pooled) (void)hipFreeAsync(p.acc, st);         // stream-ordered: behind the two kernels
  if (p.acc && !pooled) { (void)hipStreamSynchronize(st); (void)hipFree(p.acc); }
  if (le != hipSuccess) {
    mh_set_error("kernel launch failed: %s (%s:%d)", hipGetErrorString(le), __FILE__, __LINE__);
    return MH_ERR_HIP;
  }
  return MH_OK;
}

// ---- body against scene -------------------------------------------------------------------------------------------------------
#define RV_BLOCK 256

struct ReportV {
  int B, V, H, W, bpb;                // workgroups per body
  float fx, fy, cx, cy, margin;
  const float* verts;
  const float* scene_depth;
  const uint8_t* scene_mask;
  int* pen_count;
  unsigned* pen_max;                  // float bits: the values compared are positive
};

__global__ __launch_bounds__(RV_BLOCK) void k_fit_report_verts(ReportV p) {
  __shared__ int s_n;
  __shared__ unsigned s_m;
  const int tid = threadIdx.x, lane = tid & 63;
  const int b = blockIdx.x / p.bpb, v = (blockIdx.x - b * p.bpb) * RV_BLOCK + tid;
  if (tid == 0) { s_n = 0; s_m = 0u; }
  __syncthreads();
  unsigned deep = 0u;
  bool in = false;
  if (v < p.V) {
    const float* q = p.verts + ((size_t)b * p.V + v) * 3;
    const float x = q[0], y = q[1], z = q[2];
    if (z > 0.f) {
      const float fu = floorf(p.fx * x / z + p.cx), fv = floorf(p.fy * y / z + p.cy);
      if (fu >= 0.f && fu < (float)p.W && fv >= 0.f && fv < (float)p.H) {      // (false for NaN)
        const int pix = (int)fv * p.W + (int)fu;
        if (p.scene_mask[pix] != 0) {
          const float pen = z - p.scene_depth[pix];
          if (pen > p.margin) { in = true; deep = __float_as_uint(pen); }   // margin >= 0: pen > 0, its bits order like its value
        }
      }
    }
  }
  const int c = __popcll(__ballot(in));
  if (c) {                                          // (wave-uniform)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) deep = max(deep, (unsigned)__shfl_xor((int)deep, o, 64));
    if (lane == 0) { atomicAdd(&s_n, c); atomicMax(&s_m, deep); }
  }
  __syncthreads();
  if (tid == 0 && s_n != 0) {
    if (p.pen_count) atomicAdd(&p.pen_count[b], s_n);
    if (p.pen_max) atomicMax(&p.pen_max[b], s_m);
  }
}

extern "C" int mh_fit_report_verts(int B, int V, int H, int W, const float* K, const float* verts, const float* scene_depth,
                                   const uint8_t* scene_mask, float margin, int32_t* pen_count, float* pen_max, void* stream) {
  MH_CHECK(pen_count || pen_max, "no output requested (pen_count and pen_max are both null)");
  MH_CHECK(B > 0 && V > 0 && H > 0 && W > 0, "empty input");
  MH_CHECK((long long)H * W <= 0x7fffffffll && H <= (1 << 24) && W <= (1 << 24), "image too large");
  MH_CHECK(K && verts && scene_depth && scene_mask, "null argument");
  MH_CHECK(margin >= 0.f, "margin must not be negative (the maximum is taken over the bit patterns of positive floats)");
  ReportV p;
  p.B = B; p.V = V; p.H = H; p.W = W;
  p.bpb = (V + RV_BLOCK - 1) / RV_BLOCK;
  MH_CHECK((long long)B * p.bpb <= 0x7fffffffll, "too many bodies for one launch");
  p.fx = K[0]; p.cx = K[2]; p.fy = K[4]; p.cy = K[5];
  p.margin = margin;
  p.verts = verts; p.scene_depth = scene_depth; p.scene_mask = scene_mask;
  p.pen_count = pen_count; p.pen_max = (unsigned*)pen_max;
  hipStream_t st = (hipStream_t)stream;
  if (pen_count) MH_HIP(hipMemsetAsync(pen_count, 0, (size_t)B * sizeof(int32_t), st));
  if (pen_max) MH_HIP(hipMemsetAsync(pen_max, 0, (size_t)B * sizeof(float), st));
  hipLaunchKernelGGL(k_fit_report_verts, dim3((unsigned)(B * p.bpb)), dim3(RV_BLOCK), 0, st, p);
  MH_LAUNCH_CHECK();
  return MH_OK;
}
