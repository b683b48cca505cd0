// dev_buf.hip -- the memory functions behind DevBuf (dev_buf.h) over HIP, and the count of the bytes they hold.
#include <hip/hip_runtime.h>
#include <atomic>
#include "dev_buf.h"

static std::atomic<int64_t> g_live_bytes{0};

int bcx_mem_alloc(void** p, size_t bytes, bool zero, bool fine_grained) {
  *p = nullptr;
  hipError_t e = fine_grained ? hipExtMallocWithFlags(p, bytes, hipDeviceMallocFinegrained) : hipMalloc(p, bytes);
  if (e == hipSuccess && zero && (e = hipMemset(*p, 0, bytes)) != hipSuccess) (void)hipFree(*p);
  if (e != hipSuccess) { *p = nullptr; return (int)e; }
  g_live_bytes += (int64_t)bytes;
  return 0;
}

int bcx_mem_free(void* p, size_t bytes) {
  g_live_bytes -= (int64_t)bytes;
  return (int)hipFree(p);
}

int bcx_mem_copy(void* dst, const void* src, size_t bytes) { return (int)hipMemcpy(dst, src, bytes, hipMemcpyDeviceToDevice); }

int bcx_mem_copy_rows(void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, size_t rows) {
  return (int)hipMemcpy2D(dst, dpitch, src, spitch, width, rows, hipMemcpyDeviceToDevice);
}

// dev / tests: bytes of device memory that DevBufs of this process hold now; not in include/bcx.h
extern "C" int64_t bcx_debug_live_device_bytes(void) { return g_live_bytes.load(); }
