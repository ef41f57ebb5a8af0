// hip_host.h -- the host-side plumbing every C-ABI handle shares: one status path, one allocation function, one owner of a handle's
// buffers, one destroy, one stage timer and its read-out, one alignment test, one finiteness test.  Host code only; a new feature file takes these instead of writing its own.
#pragma once
#include "../../include/rgbid.h"
#include "ctx.h"

#include <cmath>
#include <utility>
#include <vector>

namespace rgbid {

// a failing HIP call is reported through the return value; the runtime's sticky "last error" is cleared so that the next launch check, or
// the caller's other HIP users (a framework sharing the process), do not trip over it later
inline int hip_status(hipError_t e) {
  if (e == hipSuccess) return RGBID_OK;
  (void)hipGetLastError();
  return (int)e;
}
#define RGBID_HIP(expr) do { if (int r_ = rgbid::hip_status(expr)) return r_; } while (0)

// device / pinned host memory; on failure *p is null, the sticky error is cleared and out-of-memory reads RGBID_E_NOMEM
inline int alloc_status(hipError_t e, void** p) {
  if (e == hipSuccess) return RGBID_OK;
  *p = nullptr;
  const int r = hip_status(e);
  return e == hipErrorOutOfMemory ? RGBID_E_NOMEM : r;
}
inline int hip_alloc(void** p, size_t bytes) { return alloc_status(hipMalloc(p, bytes), p); }
inline int hip_alloc_host(void** p, size_t bytes) { return alloc_status(hipHostMalloc(p, bytes, hipHostMallocDefault), p); }

// the buffers of one handle, held by value: whatever alloc / alloc_host handed out is freed by release() or with the handle
struct Buffers {
  std::vector<std::pair<void*, bool>> held;   // pointer, pinned
  size_t dev_bytes = 0;
  template <class T> int alloc(T** p, size_t bytes) { return take((void**)p, bytes, false); }
  template <class T> int alloc_host(T** p, size_t bytes) { return take((void**)p, bytes, true); }
  size_t bytes() const { return dev_bytes; }   // device total
  void release() {
    for (const auto& h : held) h.second ? (void)hipHostFree(h.first) : (void)hipFree(h.first);
    (void)hipGetLastError();
    held.clear();
    dev_bytes = 0;
  }
  Buffers() = default;
  Buffers(const Buffers&) = delete;
  Buffers& operator=(const Buffers&) = delete;
  ~Buffers() { release(); }

 private:
  int take(void** p, size_t bytes, bool pinned) {
    if (int r = pinned ? hip_alloc_host(p, bytes) : hip_alloc(p, bytes)) return r;
    held.push_back({*p, pinned});
    if (!pinned) dev_bytes += bytes;
    return RGBID_OK;
  }
};

// the destroy of a handle whose state is its Buffers and StageTimer: the context's stream may still read its tables, so it is drained first
template <class H>
int destroy_handle(H* h) {
  if (!h) return RGBID_OK;
  (void)hipSetDevice(h->ctx->device);
  if (h->ctx->stream) (void)hipStreamSynchronize(h->ctx->stream);
  delete h;
  return RGBID_OK;
}

// N events around the stages of a handle's calls: created on the first enable (a later enable creates what an earlier one could not),
// recorded only while enabled, destroyed with the handle -- declare it after the handle's Buffers, whose release clears the sticky error.
// Whether the LAST call was recorded is the handle's business (it copies `on` when a call has run).
template <int N>
struct StageTimer {
  bool on = false;
  hipEvent_t ev[N] = {};
  int enable(bool want) {
    if (want)
      for (hipEvent_t& e : ev) if (!e) RGBID_HIP(hipEventCreate(&e));
    on = want;
    return RGBID_OK;
  }
  void mark(int i, hipStream_t s) { if (on) (void)hipEventRecord(ev[i], s); }
  hipError_t elapsed(int a, int b, float* ms) const { return hipEventElapsedTime(ms, ev[a], ev[b]); }   // for RGBID_HIP
  StageTimer() = default;
  StageTimer(const StageTimer&) = delete;
  StageTimer& operator=(const StageTimer&) = delete;
  ~StageTimer() { for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e); }
};

// the ms[] of a *_timing call: stage k is the time between the events of pairs[k] = {a, b, c, d}, [a, b] plus [c, d] where c < d; 0 for a
// stage that the last call did not record
template <int N, int S>
int stage_times(const StageTimer<N>& t, const bool (&timed)[S], const int (&pairs)[S][4], float* ms) {
  for (int k = 0; k < S; ++k) ms[k] = 0.f;
  for (int k = 0; k < S; ++k)
    for (int j = 0; j < 4 && timed[k] && pairs[k][j] < pairs[k][j + 1]; j += 2) {
      float one = 0.f;
      RGBID_HIP(t.elapsed(pairs[k][j], pairs[k][j + 1], &one));
      ms[k] += one;
    }
  return RGBID_OK;
}

// what every C-ABI asks of a device array of 32-bit words; null passes (whether null is allowed is the caller's test)
inline bool aligned4(const void* p) { return !(((uintptr_t)p) & 3); }

// whether the n doubles of a pose, or of several, are all finite
inline bool finite_all(const double* p, int n) {
  for (int i = 0; i < n; ++i) if (!std::isfinite(p[i])) return false;
  return true;
}

}  // namespace rgbid
