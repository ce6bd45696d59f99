// Streams of the optimisation cycle and the hardware queues behind them.
//
// A captured cycle runs on three in-order queues at once: the chain on the stream the graph is launched on, the graph's
// side branch on a stream the HIP runtime creates when the graph is instantiated, and the device-side scene update
// (reference optimizer.py:578-584) on a stream of the engine's.  The runtime multiplexes all streams of a process onto a
// handful of hardware queues (GPU_MAX_HW_QUEUES, 4 by default), and two streams that land on the same hardware queue
// run one after the other: measured on MI355X (round 6, tools/fit_cycles.py), the same fit(250) takes 0.81 ms per cycle
// when the three are on three queues, 1.0 ms when the side branch shares the scene update's, 1.6 ms when it shares the
// chain's -- and which of the three it is depended on how many streams the process had created before.  These entry
// points let the host side SEE the mapping (a stream the library creates itself is a new runtime stream, placed by the
// same rule as the graph's internal one) instead of hoping.
#include "mh_common.h"

__global__ void k_spin(long long cycles, int* sink) {
  const long long t0 = (long long)wall_clock64();               // constant 100 MHz counter
  while ((long long)wall_clock64() - t0 < cycles) {
  }
  if (sink && cycles < 0) sink[0] = 1;
}

// what a call creates is destroyed on every way out of it (MH_HIP / MH_LAUNCH_CHECK return early); release() keeps it
namespace {
struct StreamGuard {
  hipStream_t s = nullptr;
  ~StreamGuard() { if (s) (void)hipStreamDestroy(s); }
  hipStream_t release() { hipStream_t r = s; s = nullptr; return r; }
};
struct EventGuard {
  hipEvent_t e = nullptr;
  ~EventGuard() { if (e) (void)hipEventDestroy(e); }
};
}  // namespace

extern "C" int mh_stream_create(void** out) {
  MH_CHECK(out, "null argument");
  StreamGuard s;
  MH_HIP(hipStreamCreateWithFlags(&s.s, hipStreamNonBlocking));
  // first submission now: the runtime binds a stream to its hardware queue when it first has work
  hipLaunchKernelGGL(k_spin, dim3(1), dim3(1), 0, s.s, 0ll, (int*)nullptr);
  MH_LAUNCH_CHECK();
  MH_HIP(hipStreamSynchronize(s.s));
  *out = (void*)s.release();
  return MH_OK;
}

extern "C" int mh_stream_destroy(void* stream) {
  MH_CHECK(stream, "null argument");
  MH_HIP(hipStreamSynchronize((hipStream_t)stream));
  MH_HIP(hipStreamDestroy((hipStream_t)stream));
  return MH_OK;
}

// one spin kernel of ~spin_us on the stream (asynchronous): occupies the stream's hardware queue, not the compute units
extern "C" int mh_stream_spin(void* stream, float spin_us) {
  MH_CHECK(spin_us > 0.f && spin_us <= 1e5f, "spin_us");
  hipLaunchKernelGGL(k_spin, dim3(1), dim3(1), 0, (hipStream_t)stream, (long long)(spin_us * 100.f), (int*)nullptr);
  MH_LAUNCH_CHECK();
  return MH_OK;
}

// Do streams a and b drain through the same hardware queue?  A spin kernel of ~spin_us on a, then an empty kernel on b:
// in a shared (in-order) queue the second ends after the first, in different queues long before it.  Synchronises both.
extern "C" int mh_streams_share_queue(void* a, void* b, float spin_us, int* shared) {
  MH_CHECK(shared, "null argument");
  MH_CHECK(spin_us > 0.f && spin_us <= 1e5f, "spin_us");
  hipStream_t sa = (hipStream_t)a, sb = (hipStream_t)b;
  if (sa == sb) { *shared = 1; return MH_OK; }
  MH_HIP(hipStreamSynchronize(sa));
  MH_HIP(hipStreamSynchronize(sb));
  EventGuard e0, ea, eb;
  MH_HIP(hipEventCreate(&e0.e)); MH_HIP(hipEventCreate(&ea.e)); MH_HIP(hipEventCreate(&eb.e));
  const long long cycles = (long long)(spin_us * 100.f);      // wall_clock64: 100 MHz
  MH_HIP(hipEventRecord(e0.e, sa));
  hipLaunchKernelGGL(k_spin, dim3(1), dim3(1), 0, sa, cycles, (int*)nullptr);
  MH_HIP(hipEventRecord(ea.e, sa));
  hipLaunchKernelGGL(k_spin, dim3(1), dim3(1), 0, sb, 0ll, (int*)nullptr);
  MH_HIP(hipEventRecord(eb.e, sb));
  MH_LAUNCH_CHECK();
  MH_HIP(hipStreamSynchronize(sa));
  MH_HIP(hipStreamSynchronize(sb));
  float ta = 0.f, tb = 0.f;
  MH_HIP(hipEventElapsedTime(&ta, e0.e, ea.e));
  const hipError_t rb = hipEventElapsedTime(&tb, e0.e, eb.e);     // (b may have finished before e0 was even recorded)
  if (rb != hipSuccess) { (void)hipGetLastError(); tb = 0.f; }
  *shared = tb >= 0.8f * ta ? 1 : 0;
  return MH_OK;
}
