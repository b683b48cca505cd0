// DevBuf<T>: the one owner of a block of device memory.  Host only, and no HIP header: the memory comes from the four
// functions below (dev_buf.hip defines them over HIP; tests/host/dev_buf_check.cpp over malloc, with allocations that fail).
#pragma once
#include <stddef.h>
#include <stdint.h>

// Each returns the HIP status as an int (0 = success), so callers word their errors as they always did.
int bcx_mem_alloc(void** p, size_t bytes, bool zero, bool fine_grained);   // *p = nullptr on failure; zero: filled with 0 bytes
int bcx_mem_free(void* p, size_t bytes);                                   // `bytes` as allocated (the live-byte count)
int bcx_mem_copy(void* dst, const void* src, size_t bytes);                // device to device
int bcx_mem_copy_rows(void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, size_t rows);   // pitches, width: bytes

template <class T> class DevBuf {
 public:
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr; o.n_ = 0; }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) { reset(); p_ = o.p_; n_ = o.n_; o.p_ = nullptr; o.n_ = 0; }
    return *this;
  }
  ~DevBuf() { reset(); }

  T* get() const { return p_; }
  operator T*() const { return p_; }
  size_t count() const { return n_; }      // elements allocated; 0 = empty
  void reset() {
    if (p_) (void)bcx_mem_free(p_, n_ * sizeof(T));
    p_ = nullptr; n_ = 0;
  }

  // `count` elements (at least one, so that a buffer in use is never null); what the buffer held is gone.  The old block is
  // freed BEFORE the new one is asked for: the largest buffers (the tier shadows) must not exist twice.  Failure: empty.
  int alloc(size_t count, bool zero, bool fine_grained = false) {
    reset();
    if (count == 0) count = 1;
    void* q = nullptr;
    const int e = bcx_mem_alloc(&q, count * sizeof(T), zero, fine_grained);
    if (e != 0) return e;
    p_ = (T*)q; n_ = count;
    return 0;
  }

  // A NEW zero-filled buffer of `new_count` elements whose first `keep` are those of `from`; `from` is not touched.
  // Failure: *status is the HIP status and the result is empty.  A *status that is not 0 on entry stays, and nothing is
  // done: a caller builds all its buffers in a row and asks once.
  static DevBuf grown(const DevBuf& from, size_t new_count, size_t keep, int* status) {
    DevBuf out;
    if (*status != 0) return out;
    *status = out.alloc(new_count, true);
    if (*status == 0 && keep) *status = bcx_mem_copy(out.p_, from.p_, keep * sizeof(T));
    if (*status != 0) out.reset();
    return out;
  }
  // The same for a row-major matrix that changes its row stride: `new_rows` x `new_ld`, the first `keep_rows` rows (of
  // `old_ld` elements each) copied into the new stride.
  static DevBuf grown_rows(const DevBuf& from, size_t old_ld, size_t new_rows, size_t new_ld, size_t keep_rows, int* status) {
    DevBuf out;
    if (*status != 0) return out;
    *status = out.alloc(new_rows * new_ld, true);
    if (*status == 0 && keep_rows && old_ld)
      *status = bcx_mem_copy_rows(out.p_, new_ld * sizeof(T), from.p_, old_ld * sizeof(T), old_ld * sizeof(T), keep_rows);
    if (*status != 0) out.reset();
    return out;
  }

 private:
  T* p_ = nullptr;
  size_t n_ = 0;
};
