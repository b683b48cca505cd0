// launch_host.h -- host-side launch plumbing of the entry points that take no bcx_solver*: reporting a HIP status (hip_fail,
// BCX_TRY), the current device's slot in a per-device cache, its CU count, the dynamic LDS a kernel may have, raising a
// kernel's dynamic-LDS limit once per device, and the size of a grid whose workgroups must be resident together.
// Host only.  Every cache is one PerDevice per kernel, a function-local static at the call site: zero means "not asked yet".
// (GridSync's set-up, grid_sync_at, sits next to the struct in csrc/nnls_common.h.)
#pragma once
#include <hip/hip_runtime.h>
#include <atomic>
#include <stddef.h>
#include <stdint.h>
#include "../../include/bcx.h"
#include "host_err.h"

// A HIP status that is not hipSuccess: the message (host_err.h) becomes "<who>: <step>: <HIP's reason>", HIP's sticky last
// error is drained so that the next entry point's hipGetLastError() does not report this failure again, and BCX_ERR_HIP is returned.
static inline int hip_fail(const char* who, const char* step, hipError_t e) {
  (void)hipGetLastError();
  return bcx_fail(BCX_ERR_HIP, who, std::string(step) + ": " + hipGetErrorString(e));
}
// `who`: the entry point (a helper that serves several passes the name it reports under); the step is the call's source text.
#define BCX_TRY(who, call)                                          \
  do {                                                              \
    const hipError_t _e = (call);                                   \
    if (_e != hipSuccess) return hip_fail(who, #call, _e);          \
  } while (0)

#define BCX_MAX_DEVICES 64
template <class T> struct PerDevice { std::atomic<T> of[BCX_MAX_DEVICES]; };

// The current device's index into a PerDevice, in the two forms the callers need: -1 without a device (or one past the
// caches), for questions that have no answer then; slot 0, for caches whose caller goes on to a launch that reports the error.
static inline int device_slot_or_fail() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= BCX_MAX_DEVICES) return -1;
  return dev;
}
static inline int device_slot_or_zero() {
  const int dev = device_slot_or_fail();
  return dev < 0 ? 0 : dev;
}

// CUs of the current device, asked once per device.  A query that fails answers 256 (an MI355X), is not cached, and leaves
// no HIP error behind: the plans that size scratch and the launches that use it then still agree.
inline int cu_count() {
  static PerDevice<int> cache;
  const int dev = device_slot_or_fail();
  int cus = dev < 0 ? 0 : cache.of[dev].load(std::memory_order_relaxed);
  if (cus > 0) return cus;
  if (dev >= 0 && hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && cus > 0) {
    cache.of[dev].store(cus, std::memory_order_relaxed);
    return cus;
  }
  (void)hipGetLastError();
  return 256;
}

// dynamic LDS one workgroup of `kernel` may have on the current device: the device's limit minus the kernel's static use
// (-1: no device, or a query failed -- that is not cached)
static inline int64_t lds_room(const void* kernel, PerDevice<int64_t>& cache) {
  const int dev = device_slot_or_fail();
  if (dev < 0) return -1;
  int64_t r = cache.of[dev].load(std::memory_order_acquire);
  if (r != 0) return r;
  int maxb = 0;
  hipFuncAttributes fa;
  if (hipDeviceGetAttribute(&maxb, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) != hipSuccess ||
      hipFuncGetAttributes(&fa, kernel) != hipSuccess) {
    (void)hipGetLastError();
    return -1;
  }
  r = (int64_t)maxb - (int64_t)fa.sharedSizeBytes;
  if (r <= 0) r = -1;
  cache.of[dev].store(r, std::memory_order_release);
  return r;
}

// Let `kernel` have `bytes` of dynamic LDS.  Nothing to do at or below `threshold` (what a kernel may have unasked) or at or
// below the largest request so far on the current device; else the attribute is raised and the request remembered.  The caller
// reports a failure under its own name (BCX_TRY).
static inline hipError_t raise_dynamic_lds(const void* kernel, size_t bytes, size_t threshold, PerDevice<size_t>& cache) {
  if (bytes <= threshold) return hipSuccess;
  std::atomic<size_t>& largest = cache.of[device_slot_or_zero()];
  if (bytes <= largest.load(std::memory_order_acquire)) return hipSuccess;
  const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  if (e == hipSuccess) largest.store(bytes, std::memory_order_release);
  return e;
}

// Workgroups of `kernel` (`threads` threads, no dynamic LDS) that are resident together on the current device: one per CU, when
// the occupancy query admits one; -1: none (cached like an answer).
static inline int one_wg_per_cu(const void* kernel, int threads, PerDevice<int>& cache) {
  const int dev = device_slot_or_zero();
  int n = cache.of[dev].load(std::memory_order_acquire);
  if (n != 0) return n;
  int per_cu = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, threads, 0) != hipSuccess) (void)hipGetLastError();
  n = per_cu < 1 ? -1 : cu_count();                   // (the query over-reports for some kernels; one per CU keeps a margin)
  cache.of[dev].store(n, std::memory_order_release);
  return n;
}
