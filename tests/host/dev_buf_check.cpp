// Host check of csrc/dev_buf.h (tests/test_dev_buf_host.py builds it with -fsanitize=address,undefined and runs it).
// "Device" memory is malloc here; the n-th allocation can be made to fail, and every byte handed out is counted.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <utility>
#include <vector>
#include "../../bayesian-coresets_amd/csrc/dev_buf.h"

static long long g_live = 0;           // bytes allocated and not freed
static long long g_live_at_alloc = 0;  // g_live when the last allocation was asked for
static int g_allocs = 0;               // allocations asked for since the last arm()
static int g_fail_at = 0;              // 1-based: that allocation fails; 0: none
static void arm(int fail_at) { g_allocs = 0; g_fail_at = fail_at; }

int bcx_mem_alloc(void** p, size_t bytes, bool zero, bool) {
  *p = nullptr;
  g_live_at_alloc = g_live;
  if (++g_allocs == g_fail_at) return 2;   // (hipErrorOutOfMemory)
  void* q = malloc(bytes);
  if (!q) return 2;
  memset(q, zero ? 0 : 0xA5, bytes);       // an unfilled block is visibly not zero
  g_live += (long long)bytes;
  *p = q;
  return 0;
}
int bcx_mem_free(void* p, size_t bytes) { g_live -= (long long)bytes; free(p); return 0; }
int bcx_mem_copy(void* dst, const void* src, size_t bytes) { memcpy(dst, src, bytes); return 0; }
int bcx_mem_copy_rows(void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, size_t rows) {
  for (size_t r = 0; r < rows; ++r) memcpy((char*)dst + r * dpitch, (const char*)src + r * spitch, width);
  return 0;
}

static int g_failed = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); g_failed += 1; } } while (0)

template <class T> static std::vector<T> snapshot(const DevBuf<T>& b) { return std::vector<T>(b.get(), b.get() + b.count()); }

static void test_moves_and_reset() {
  const long long live0 = g_live;
  DevBuf<double> a;
  CHECK(a.get() == nullptr && a.count() == 0 && !a);
  CHECK(a.alloc(10, true) == 0);
  CHECK(a.count() == 10 && g_live == live0 + 80);
  double* p = a.get();
  CHECK((double*)a == p);
  DevBuf<double> b(std::move(a));                          // move construction: the block changes hands, nothing is copied or freed
  CHECK(b.get() == p && b.count() == 10 && a.get() == nullptr && a.count() == 0 && g_live == live0 + 80);
  DevBuf<double> c;
  CHECK(c.alloc(3, true) == 0);
  CHECK(g_live == live0 + 80 + 24);
  c = std::move(b);                                        // move assignment frees what the target held
  CHECK(c.get() == p && c.count() == 10 && b.get() == nullptr && g_live == live0 + 80);
  DevBuf<double>& cref = c;
  c = std::move(cref);                                     // onto itself: unchanged
  CHECK(c.get() == p && c.count() == 10 && g_live == live0 + 80);
  c.reset();
  CHECK(c.get() == nullptr && c.count() == 0 && g_live == live0);
  c.reset();                                               // twice is harmless
  CHECK(g_live == live0);
  {
    DevBuf<int32_t> d;
    CHECK(d.alloc(5, false) == 0);
    CHECK(g_live == live0 + 20);
  }                                                        // the destructor frees
  CHECK(g_live == live0);
}

static void test_alloc() {
  const long long live0 = g_live;
  DevBuf<unsigned char> a;
  CHECK(a.alloc(64, true) == 0);
  for (size_t i = 0; i < 64; ++i) CHECK(a[i] == 0);                       // zero-fill on
  CHECK(a.alloc(1000, false) == 0);
  CHECK(g_live_at_alloc == live0);                         // the 64 bytes were gone when the 1000 were asked for
  CHECK(a.count() == 1000 && g_live == live0 + 1000);
  for (size_t i = 0; i < 1000; ++i) CHECK(a[i] == 0xA5);                  // zero-fill off: left as the allocator gave it
  arm(1);
  CHECK(a.alloc(2000, true) != 0);                         // failure: empty, and the old block is gone
  arm(0);
  CHECK(a.get() == nullptr && a.count() == 0 && g_live == live0);
  CHECK(a.alloc(0, true) == 0);                            // never null after a successful alloc
  CHECK(a.get() != nullptr && a.count() == 1 && g_live == live0 + 1);
}

static void test_grown() {
  const long long live0 = g_live;
  DevBuf<int64_t> a;
  CHECK(a.alloc(8, true) == 0);
  for (int i = 0; i < 8; ++i) a[i] = 100 + i;
  const std::vector<int64_t> was = snapshot(a);
  int e = 0;
  DevBuf<int64_t> b = DevBuf<int64_t>::grown(a, 20, 5, &e);
  CHECK(e == 0 && b.count() == 20 && b.get() != a.get());
  for (int i = 0; i < 20; ++i) CHECK(b[i] == (i < 5 ? 100 + i : 0));      // exactly `keep` elements, zeros behind them
  CHECK(snapshot(a) == was && a.count() == 8);
  CHECK(g_live == live0 + 8 * 8 + 20 * 8);
  DevBuf<int64_t> none;
  DevBuf<int64_t> c = DevBuf<int64_t>::grown(none, 4, 0, &e);             // from nothing
  CHECK(e == 0 && c.count() == 4 && c[0] == 0 && c[3] == 0);
  arm(1);
  DevBuf<int64_t> f = DevBuf<int64_t>::grown(a, 20, 5, &e);
  arm(0);
  CHECK(e != 0 && f.get() == nullptr && f.count() == 0 && snapshot(a) == was);
  const long long live_failed = g_live;
  DevBuf<int64_t> f2 = DevBuf<int64_t>::grown(a, 20, 5, &e);              // a status that already failed stays: nothing is done
  CHECK(e != 0 && f2.get() == nullptr && g_allocs == 0 && g_live == live_failed);
  e = 0;

  // pitched: 3 x 3 at stride 3 into 5 x 5 at stride 5, two rows kept
  DevBuf<double> m;
  CHECK(m.alloc(9, true) == 0);
  for (int i = 0; i < 9; ++i) m[i] = 1.0 + i;
  const std::vector<double> mwas = snapshot(m);
  DevBuf<double> g = DevBuf<double>::grown_rows(m, 3, 5, 5, 2, &e);
  CHECK(e == 0 && g.count() == 25);
  for (int r = 0; r < 5; ++r)
    for (int c2 = 0; c2 < 5; ++c2) CHECK(g[r * 5 + c2] == ((r < 2 && c2 < 3) ? 1.0 + r * 3 + c2 : 0.0));
  CHECK(snapshot(m) == mwas);
  DevBuf<double> g0 = DevBuf<double>::grown_rows(DevBuf<double>(), 0, 4, 4, 0, &e);   // from nothing
  CHECK(e == 0 && g0.count() == 16 && g0[15] == 0.0);
}

// A capacity change in the pattern of the solver's (api.hip): every new buffer in a local, then one block that cannot fail.
struct Owner {
  DevBuf<int64_t> idx;      // preserved
  DevBuf<double> gram;      // preserved, cap x cap
  DevBuf<int32_t> flag;     // scratch
  size_t cap = 0;
};
static int ensure(Owner& o, size_t ncap) {
  int e = 0;
  auto idx = DevBuf<int64_t>::grown(o.idx, ncap, o.cap, &e);
  auto gram = DevBuf<double>::grown_rows(o.gram, o.cap, ncap, ncap, o.cap, &e);
  auto flag = DevBuf<int32_t>::grown(o.flag, ncap, 0, &e);
  if (e) return e;
  o.idx = std::move(idx); o.gram = std::move(gram); o.flag = std::move(flag);
  o.cap = ncap;
  return 0;
}

static void test_commit() {
  const long long live0 = g_live;
  {
    Owner o;
    CHECK(ensure(o, 4) == 0 && o.cap == 4);
    for (int i = 0; i < 4; ++i) { o.idx[i] = 7 * i + 1; o.flag[i] = -i; }
    for (int i = 0; i < 16; ++i) o.gram[i] = 0.5 * i;
    const std::vector<int64_t> idx_was = snapshot(o.idx);
    const std::vector<double> gram_was = snapshot(o.gram);
    const std::vector<int32_t> flag_was = snapshot(o.flag);
    const int64_t* pi = o.idx.get(); const double* pg = o.gram.get(); const int32_t* pf = o.flag.get();
    const long long live1 = g_live;
    int n_allocs = 0;
    for (int n = 1; ; ++n) {                   // a failure at allocation n, for every n the commit makes
      arm(n);
      const int e = ensure(o, 9);
      const bool reached = g_allocs >= n;
      arm(0);
      if (!reached) { CHECK(e == 0); n_allocs = n - 1; break; }
      CHECK(e != 0);
      CHECK(o.cap == 4 && o.idx.get() == pi && o.gram.get() == pg && o.flag.get() == pf);
      CHECK(snapshot(o.idx) == idx_was && snapshot(o.gram) == gram_was && snapshot(o.flag) == flag_was);
      CHECK(g_live == live1);
    }
    CHECK(n_allocs == 3);
    CHECK(o.cap == 9 && o.idx.count() == 9 && o.gram.count() == 81 && o.flag.count() == 9);
    for (int i = 0; i < 9; ++i) CHECK(o.idx[i] == (i < 4 ? idx_was[i] : 0) && o.flag[i] == 0);
    for (int r = 0; r < 9; ++r)
      for (int c = 0; c < 9; ++c) CHECK(o.gram[r * 9 + c] == ((r < 4 && c < 4) ? gram_was[r * 4 + c] : 0.0));
    CHECK(g_live == live0 + 9 * 8 + 81 * 8 + 9 * 4);
  }
  CHECK(g_live == live0);
}

int main() {
  test_moves_and_reset();
  test_alloc();
  test_grown();
  test_commit();
  CHECK(g_live == 0);
  if (g_failed) { printf("%d CHECKS FAILED\n", g_failed); return 1; }
  printf("DEV_BUF OK\n");
  return 0;
}
