// Test infrastructure (tests/stream_probe.py, tests/test_gpu_stream_order.py), not part of the
// C-ABI: what the suite needs to hold one stream of a context back while the host enqueues the calls
// whose cross-stream ordering is under test.
//
//   - a delay: one wave that spins on the fixed-rate device clock (wall_clock64) for a requested number
//     of microseconds, launched on a given stream and followed by an event record, which is the token.
//     Bounded twice: the request is clamped to kMaxDelayUs, and the loop ends after a number of
//     iterations proportional to the request even if the clock never advances.  It reads and writes no
//     memory: no flag, no gate the host releases, nothing polled.
//   - pending(token): hipEventQuery on the token, and a release that destroys it.
//   - a read-only door to a single-table context's three stream handles (fm_context.h).
//
// Compiled into the sort probe's library, beside the built libfm_hip.so it is linked against.  No
// exception crosses the boundary.
#include <hip/hip_runtime.h>

#include <mutex>

#include "../../fm_spark_amd/csrc/fm_context.h"

namespace {

constexpr int64_t kMaxDelayUs = 200000;  // 200 ms
// One iteration sleeps 32 * 64 clocks (about a microsecond) and reads the clock once, so 16 iterations
// per requested microsecond never end a delay early, and end one within a few seconds whatever the
// clock does.
constexpr int64_t kItersPerUs = 16;
constexpr int64_t kItersFloor = 4096;

__global__ void k_stream_delay(long long ticks, long long max_iters) {
  const long long t0 = wall_clock64();
  for (long long i = 0; i < max_iters; ++i) {
    if (wall_clock64() - t0 >= ticks) break;
    __builtin_amdgcn_s_sleep(32);
  }
}

}  // namespace

extern "C" {

// the longest delay a request is clamped to, in microseconds
int64_t stream_probe_max_delay_us(void) { return kMaxDelayUs; }

// a delay of min(us, kMaxDelayUs) microseconds enqueued on `stream` (a hipStream_t; NULL: the null
// stream), then an event recorded behind it: *token.  The caller releases the token.
int stream_probe_delay(void* stream, int64_t us, void** token) {
  if (!token || us < 0) return FM_ERR_ARG;
  *token = nullptr;
  us = us > kMaxDelayUs ? kMaxDelayUs : us;
  int dev = 0, khz = 0;
  if (hipGetDevice(&dev) != hipSuccess) return FM_ERR_HIP;
  if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev) != hipSuccess || khz <= 0) return FM_ERR_HIP;
  const long long ticks = (long long)(us * (int64_t)khz / 1000);
  const long long max_iters = (long long)(us * kItersPerUs + kItersFloor);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipEvent_t ev = nullptr;
  if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) return FM_ERR_HIP;
  k_stream_delay<<<dim3(1), dim3(64), 0, st>>>(ticks, max_iters);
  if (hipGetLastError() != hipSuccess || hipEventRecord(ev, st) != hipSuccess) {
    (void)hipEventDestroy(ev);
    return FM_ERR_HIP;
  }
  *token = ev;
  return FM_OK;
}

// 1: the delay (and whatever the stream held before it) has not finished; 0: it has; < 0: an error
int stream_probe_pending(void* token) {
  if (!token) return FM_ERR_ARG;
  const hipError_t e = hipEventQuery(reinterpret_cast<hipEvent_t>(token));
  if (e == hipSuccess) return 0;
  if (e == hipErrorNotReady) {
    (void)hipGetLastError();  // not an error: nothing is left behind for the next launch check
    return 1;
  }
  return FM_ERR_HIP;
}

// waits for the token, then destroys it
void stream_probe_release(void* token) {
  if (!token) return;
  (void)hipEventSynchronize(reinterpret_cast<hipEvent_t>(token));
  (void)hipEventDestroy(reinterpret_cast<hipEvent_t>(token));
}

// out3 = {main, side, copy} stream handles of a single-table context as they stand now (the copy
// stream is NULL until the first call that uses it has created it)
int stream_probe_ctx_streams(void* ctx_handle, void** out3) {
  fm_ctx* ctx = reinterpret_cast<fm_ctx*>(ctx_handle);
  if (!ctx || !out3 || ctx->group) return FM_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  out3[0] = ctx->stream;
  out3[1] = ctx->side;
  out3[2] = ctx->copy_stream;
  return FM_OK;
}

}  // extern "C"
