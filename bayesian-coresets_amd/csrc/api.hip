// api.hip -- host side of the C ABI declared in include/bcx.h.
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <cmath>
#include "bcx_internal.h"
#include "dev_util.h"

static thread_local std::string g_create_err;
namespace {   // pinned upload buffers, one pair per device (defined with the upload code below)
void bounce_acquire(int device);
void bounce_release(int device);
}

extern "C" const char* bcx_version(void) { return "bcx 0.1 gfx950"; }

extern "C" const char* bcx_last_error(const bcx_solver* s) { return s ? s->err.c_str() : g_create_err.c_str(); }

static int round_up(int x, int m) { return (x + m - 1) / m * m; }

// a failed DevBuf call (its HIP status) as the solver's error, in BCX_HIP's form
static int mem_fail(bcx_solver* s, const char* what, int e) {
  s->err = std::string(what) + ": " + hipGetErrorString((hipError_t)e);
  return BCX_ERR_HIP;
}

extern "C" int bcx_create(const bcx_config* cfg, bcx_solver** out) {
  if (!cfg || !out) { g_create_err = "bcx_create: null argument"; return BCX_ERR_ARG; }
  *out = nullptr;
  if (cfg->alg < BCX_ALG_GIGA || cfg->alg > BCX_ALG_OMP || cfg->d < 1 || cfg->n_local < 0 ||
      cfg->world_size < 1 || cfg->rank < 0 || cfg->rank >= cfg->world_size ||
      (cfg->store_dtype != BCX_F32 && cfg->store_dtype != BCX_F64 && cfg->store_dtype != BCX_F16)) {
    g_create_err = "bcx_create: invalid configuration";
    return BCX_ERR_ARG;
  }
  const int maxd = BCX_MAX_D;
  if (cfg->d > maxd) { g_create_err = "bcx_create: d exceeds the supported row length (" + std::to_string(maxd) + ")"; return BCX_ERR_ARG; }
  if (cfg->n_local >= (int64_t)0x7fffffff) { g_create_err = "bcx_create: n_local must be < 2^31 per shard"; return BCX_ERR_ARG; }
  if (cfg->row_offset % BCX_CHUNK_ROWS != 0) {
    g_create_err = "bcx_create: row_offset must be a multiple of the chunk size (1024 rows)";
    return BCX_ERR_ARG;
  }
  bcx_solver* s = new bcx_solver();
  s->cfg = *cfg;
  if (s->cfg.refresh_every == 0) s->cfg.refresh_every = 64;
  if (const char* e = bcx_dev_env("BCX_SCREEN8")) s->scr_enabled = atoi(e) != 0;   // dev: 0 = the parent's path (storage-precision scan only)
  if (const char* e = bcx_dev_env("BCX_SCREEN4_SEGCAP")) { const int v = atoi(e); if (v >= 1 && v <= BCX_S4_SEG_CAP) s->s4_seg_cap = v; }   // dev: a small list segment, so that small inputs fill it
  if (const char* e = bcx_dev_env("BCX_SCREEN4")) s->s4_enabled = atoi(e) != 0;   // dev: 0 = the 8-bit tier alone, as before the 4-bit front pass
  hipError_t e = hipSetDevice(cfg->device);
  if (e != hipSuccess) { g_create_err = std::string("hipSetDevice: ") + hipGetErrorString(e); delete s; return BCX_ERR_HIP; }
  const int d = cfg->d;
  const int64_t n = cfg->n_local;
  s->elem = cfg->store_dtype == BCX_F32 ? 4 : (cfg->store_dtype == BCX_F16 ? 2 : 8);
  s->qelem = cfg->store_dtype == BCX_F64 ? 8 : 4;   // the query the scan reads: fp32 for fp32/fp16 rows
  s->ld = round_up(d, 16 / s->elem);
  s->ld64 = round_up(d, 2);
  s->n_chunks = (n + BCX_CHUNK_ROWS - 1) / BCX_CHUNK_ROWS;
  bool ok = true;
  auto chk = [&](int r) { if (r != 0 && ok) { ok = false; g_create_err = std::string("hipMalloc: ") + hipGetErrorString((hipError_t)r); } };
  chk(s->An.alloc((size_t)n * s->ld * s->elem, true));
  if (cfg->keep_exact_rows && cfg->store_dtype != BCX_F64) chk(s->A64.alloc((size_t)n * s->ld64, true));
  chk(s->norms.alloc((size_t)n, true));
  chk(s->chunk_sums.alloc((size_t)s->n_chunks * (d + 1), true));
  chk(s->st.alloc(1, true));
  chk(s->b.alloc((size_t)d, true));
  chk(s->bn.alloc((size_t)d, true));
  chk(s->xw.alloc((size_t)d, true));
  chk(s->q64.alloc((size_t)2 * s->ld64, true));
  chk(s->qst.alloc((size_t)2 * s->ld * s->qelem, true));
  chk(s->tmp.alloc((size_t)20 * d, true));
  s->n_partials = 0;
  chk(s->partials.alloc((size_t)bcx_scan_grid(s) * BCX_PARTIAL_BYTES, true));
  chk(s->rec_local.alloc((size_t)(d + BCX_REC_HDR), true));
  if (!ok) { delete s; return BCX_ERR_NOMEM; }
  bounce_acquire(cfg->device);
  *out = s;
  return BCX_OK;
}

extern "C" int bcx_destroy(bcx_solver* s) {
  if (!s) return BCX_OK;
  (void)hipSetDevice(s->cfg.device);
  (void)hipDeviceSynchronize();
  const int device = s->cfg.device;
  delete s;      // unmaps the peers' mailboxes, frees every device buffer, destroys the profiling events
  bounce_release(device);
  return BCX_OK;
}

extern "C" int bcx_set_stream(bcx_solver* s, void* hip_stream) {
  if (!s) return BCX_ERR_ARG;
  s->stream = (hipStream_t)hip_stream;
  return BCX_OK;
}

static int read_state(bcx_solver* s, DevState* h);

// ---- host -> device upload --------------------------------------------------------------------------
// The GPU never touches the caller's memory: rows are copied by host threads into two pinned bounce buffers that
// the library owns (hipHostMalloc, allocated once per process) and DMA'd from there, the memcpy of one buffer
// overlapping the DMA of the other.  (Round 1 pinned the caller's ndarray with hipHostRegister for the duration
// of the copy; on a fresh box that path died intermittently with "Memory access fault by GPU ... Reason: Unknown"
// at an address inside the registered heap range -- a user-pointer mapping of glibc heap pages is only as stable
// as the heap is -- and took the whole GPU test run with it.)  On return the caller's buffer is no longer in use.
#include <mutex>
#include <thread>
namespace {
constexpr size_t kBounceBytes = (size_t)32 << 20;
constexpr int kMaxDevices = 64;
// One pair of pinned buffers and one lock PER DEVICE: uploads to different GPUs of one process run side by side (round 2
// had a single process-wide pair: solvers on different devices queued behind each other); the pair is freed when the
// last solver of its device is destroyed.
struct Bounce {
  std::mutex mu;
  void* buf[2] = {nullptr, nullptr};
  int users = 0;
};
Bounce g_bounce[kMaxDevices];
Bounce& bounce_of(int device) { return g_bounce[(device >= 0 && device < kMaxDevices) ? device : 0]; }
void bounce_acquire(int device) {
  Bounce& b = bounce_of(device);
  std::lock_guard<std::mutex> lock(b.mu);
  b.users += 1;
}
void bounce_release(int device) {
  Bounce& b = bounce_of(device);
  std::lock_guard<std::mutex> lock(b.mu);
  if (--b.users <= 0) {
    b.users = 0;
    for (int i = 0; i < 2; ++i)
      if (b.buf[i]) { (void)hipHostFree(b.buf[i]); b.buf[i] = nullptr; }
  }
}

void copy_rows_mt(char* dst, size_t dpitch, const char* src, size_t spitch, size_t width, int64_t rows) {
  const size_t bytes = (size_t)rows * width;
  int nt = (int)std::min<size_t>(8, bytes / ((size_t)2 << 20));      // one thread per 2 MiB, at most 8
  const unsigned hw = std::thread::hardware_concurrency();
  if (hw && (unsigned)nt > hw) nt = (int)hw;
  auto work = [=](int64_t r0, int64_t r1) {
    if (dpitch == width && spitch == width) { memcpy(dst + (size_t)r0 * width, src + (size_t)r0 * width, (size_t)(r1 - r0) * width); return; }
    for (int64_t r = r0; r < r1; ++r) memcpy(dst + (size_t)r * dpitch, src + (size_t)r * spitch, width);
  };
  if (nt <= 1) { work(0, rows); return; }
  std::vector<std::thread> th;
  const int64_t per = (rows + nt - 1) / nt;
  for (int t = 1; t < nt; ++t) {
    const int64_t r0 = std::min<int64_t>(rows, t * per), r1 = std::min<int64_t>(rows, (t + 1) * per);
    if (r0 < r1) th.emplace_back(work, r0, r1);
  }
  work(0, std::min<int64_t>(rows, per));
  for (auto& t : th) t.join();
}
}  // namespace

static int upload_host_rows(bcx_solver* s, void* dst_dev, size_t dpitch, const void* src, size_t spitch, size_t width,
                            int64_t rows) {
  if (rows <= 0) return BCX_OK;
  Bounce& g_b = bounce_of(s->cfg.device);
  std::lock_guard<std::mutex> lock(g_b.mu);
  for (int i = 0; i < 2; ++i)
    if (!g_b.buf[i]) BCX_HIP(hipHostMalloc(&g_b.buf[i], kBounceBytes, hipHostMallocPortable));
  if (width > kBounceBytes) { s->err = "bcx_load_rows: a row exceeds the upload buffer"; return BCX_ERR_ARG; }
  hipEvent_t done[2] = {nullptr, nullptr};     // (per call: events belong to the device that is current now)
  bool busy[2] = {false, false};
  for (int i = 0; i < 2; ++i) {
    const hipError_t ee = hipEventCreateWithFlags(&done[i], hipEventDisableTiming);
    if (ee != hipSuccess) {
      if (i == 1) (void)hipEventDestroy(done[0]);
      s->err = std::string("upload: ") + hipGetErrorString(ee);
      return BCX_ERR_HIP;
    }
  }
  const int64_t rows_per = std::max<int64_t>(1, (int64_t)(kBounceBytes / width));
  int which = 0;
  int rc = BCX_OK;
  for (int64_t r = 0; r < rows && rc == BCX_OK; r += rows_per, which ^= 1) {
    const int64_t m = std::min(rows_per, rows - r);
    if (busy[which]) {
      if (hipEventSynchronize(done[which]) != hipSuccess) { s->err = "upload: event wait failed"; rc = BCX_ERR_HIP; break; }
      busy[which] = false;
    }
    copy_rows_mt((char*)g_b.buf[which], width, (const char*)src + (size_t)r * spitch, spitch, width, m);
    hipError_t e = hipMemcpy2DAsync((char*)dst_dev + (size_t)r * dpitch, dpitch, g_b.buf[which], width, width, (size_t)m,
                                    hipMemcpyHostToDevice, s->stream);
    if (e == hipSuccess) e = hipEventRecord(done[which], s->stream);
    if (e != hipSuccess) { s->err = std::string("upload: ") + hipGetErrorString(e); rc = BCX_ERR_HIP; break; }
    busy[which] = true;
  }
  // the bounce buffers are shared by every solver of the device: leave them idle
  for (int i = 0; i < 2; ++i) {
    if (busy[i]) (void)hipEventSynchronize(done[i]);
    (void)hipEventDestroy(done[i]);
  }
  return rc;
}


static int load_rows(bcx_solver* s, const void* src, int32_t src_is_device, int32_t src_dtype, int64_t row_begin,
                     int64_t rows, int64_t ld, int32_t flags);

extern "C" int bcx_load_rows(bcx_solver* s, const void* src, int32_t src_is_device, int32_t src_dtype,
                             int64_t row_begin, int64_t rows, int64_t ld) {
  return load_rows(s, src, src_is_device, src_dtype, row_begin, rows, ld, 0);
}

extern "C" int bcx_load_rows_flags(bcx_solver* s, const void* src, int32_t src_is_device, int32_t src_dtype,
                                   int64_t row_begin, int64_t rows, int64_t ld, int32_t flags) {
  if (flags & ~BCX_LOAD_CENTER_ROWS) { if (s) s->err = "bcx_load_rows_flags: unknown flag"; return BCX_ERR_ARG; }
  return load_rows(s, src, src_is_device, src_dtype, row_begin, rows, ld, flags);
}

static int load_rows(bcx_solver* s, const void* src, int32_t src_is_device, int32_t src_dtype, int64_t row_begin,
                     int64_t rows, int64_t ld, int32_t flags) {
  if (!s || (!src && rows > 0)) return BCX_ERR_ARG;
  const int center = (flags & BCX_LOAD_CENTER_ROWS) ? 1 : 0;
  const int d = s->cfg.d;
  if (rows == 0) return BCX_OK;
  if (row_begin < 0 || rows < 0 || row_begin + rows > s->cfg.n_local || ld < d ||
      (src_dtype != BCX_F32 && src_dtype != BCX_F64)) {
    s->err = "bcx_load_rows: bad range, leading dimension or dtype";
    return BCX_ERR_ARG;
  }
  if (row_begin % BCX_CHUNK_ROWS != 0 || (rows % BCX_CHUNK_ROWS != 0 && row_begin + rows != s->cfg.n_local)) {
    s->err = "bcx_load_rows: pieces must start and end on 1024-row chunk boundaries (except the last)";
    return BCX_ERR_ARG;
  }
  BCX_HIP(hipSetDevice(s->cfg.device));
  if (row_begin == 0) {
    // a (re)load from the first row starts a new matrix: forget the previous one's zero-row flag and state.
    // Unconditionally -- a matrix whose bcx_finalize reported BCX_ERR_ZERO_ROW never became `finalized`, and its
    // flag must not outlive it (SparseVI reloads one engine with a fresh projection every step).
    if (s->finalized || s->rows_loaded > 0) {
      DevState h;
      int rc0 = read_state(s, &h);
      if (rc0 != BCX_OK) return rc0;
      h.zero_row = 0; h.k = 0; h.np = 0; h.hvalid = 1; h.omp_ill = 0; h.limit = 0; h.active = 0; h.halt = HALT_NONE;
      BCX_HIP(hipMemcpy(s->st, &h, sizeof h, hipMemcpyHostToDevice));
      s->finalized = false;
    }
    s->rows_loaded = 0;
  }
  const size_t esz = src_dtype == BCX_F64 ? 8 : 4;
  if (src_is_device) {
    int rc = bcx_launch_ingest(s, src, src_dtype, ld, row_begin, rows, center);
    if (rc != BCX_OK) return rc;
  } else if (s->A64 && src_dtype == BCX_F64) {
    // host fp64 rows go straight to their final place; the ingest kernel then works in place
    double* dst = s->A64 + (size_t)row_begin * s->ld64;
    int rc = upload_host_rows(s, dst, (size_t)s->ld64 * 8, src, (size_t)ld * 8, (size_t)d * 8, rows);
    if (rc != BCX_OK) return rc;
    rc = bcx_launch_ingest(s, dst, BCX_F64, s->ld64, row_begin, rows, center);
    if (rc != BCX_OK) return rc;
  } else {
    // stage through a device buffer in pieces of <= 256 MiB
    const int64_t piece = std::max<int64_t>(BCX_CHUNK_ROWS,
                                            ((int64_t)(256u << 20) / (int64_t)(d * esz)) / BCX_CHUNK_ROWS * BCX_CHUNK_ROWS);
    const size_t need = (size_t)std::min(piece, rows) * d * esz;
    if (s->staging.count() < need) BCX_HIP((hipError_t)s->staging.alloc(need, false));
    for (int64_t r = 0; r < rows; r += piece) {
      const int64_t m = std::min(piece, rows - r);
      int rc = upload_host_rows(s, s->staging.get(), (size_t)d * esz, (const char*)src + (size_t)r * ld * esz, (size_t)ld * esz,
                                (size_t)d * esz, m);
      if (rc != BCX_OK) return rc;
      rc = bcx_launch_ingest(s, s->staging.get(), src_dtype, d, row_begin + r, m, center);
      if (rc != BCX_OK) return rc;
      BCX_HIP(hipStreamSynchronize(s->stream));  // staging buffer is reused
    }
  }
  s->rows_loaded += rows;
  s->scr_valid = false;      // the shadows (screen8.hip, screen4.hip) are rebuilt from the new rows before the next enqueued iteration
  s->s4_valid = false;
  return BCX_OK;
}

extern "C" int bcx_chunk_sums(bcx_solver* s, const void** dev_ptr, int64_t* n_chunks, int64_t* chunk_rows) {
  if (!s) return BCX_ERR_ARG;
  if (dev_ptr) *dev_ptr = s->chunk_sums;
  if (n_chunks) *n_chunks = s->n_chunks;
  if (chunk_rows) *chunk_rows = BCX_CHUNK_ROWS;
  return BCX_OK;
}

extern "C" int bcx_export_chunk_sums(bcx_solver* s, void* dst_dev, int64_t cap_chunks) {
  if (!s || !dst_dev || cap_chunks < s->n_chunks) return BCX_ERR_ARG;
  BCX_HIP(hipMemcpyAsync(dst_dev, s->chunk_sums, (size_t)s->n_chunks * (s->cfg.d + 1) * 8, hipMemcpyDeviceToDevice,
                         s->stream));
  return BCX_OK;
}

static int read_state(bcx_solver* s, DevState* h) {
  BCX_HIP(hipStreamSynchronize(s->stream));
  BCX_HIP(hipMemcpy(h, s->st, sizeof(DevState), hipMemcpyDeviceToHost));
  return BCX_OK;
}

extern "C" int bcx_finalize(bcx_solver* s, const double* b_host, const void* gathered_sums_dev, int64_t n_gathered) {
  if (!s) return BCX_ERR_ARG;
  BCX_HIP(hipSetDevice(s->cfg.device));
  if (s->rows_loaded < s->cfg.n_local) { s->err = "bcx_finalize: not all rows were loaded"; return BCX_ERR_STATE; }
  if (b_host) BCX_HIP(hipMemcpyAsync(s->b, b_host, (size_t)s->cfg.d * 8, hipMemcpyHostToDevice, s->stream));
  int rc = bcx_launch_finalize(s, b_host != nullptr, (const double*)gathered_sums_dev, n_gathered);
  if (rc != BCX_OK) return rc;
  DevState h;
  rc = read_state(s, &h);
  if (rc != BCX_OK) return rc;
  if (h.zero_row != 0) {
    char buf[128];
    snprintf(buf, sizeof buf, "A must not have any 0 columns (local row %d has zero norm)", h.zero_row - 1);
    s->err = buf;
    return BCX_ERR_ZERO_ROW;
  }
  if (s->cfg.alg == BCX_ALG_GIGA && h.bnorm == 0.0) { s->err = "norm of b must be > 0"; return BCX_ERR_ZERO_B; }
  s->finalized = true;
  return BCX_OK;
}

// ---- capacity management -----------------------------------------------------------------
// A capacity change commits whole or not at all: every new buffer is built in a local (DevBuf::grown: zero-filled, with a
// copy of what the kernels still read), and only when all of them exist are they moved into the solver and the capacity
// set -- a block that cannot fail.  After a failure the solver is what it was and the locals have freed what they held.
static int ensure_slots(bcx_solver* s, int64_t need) {
  if (need <= s->cap) return BCX_OK;
  const int64_t ncap = std::max<int64_t>(need, std::max<int64_t>(256, s->cap * 2));
  const size_t d = (size_t)s->cfg.d, oc = (size_t)s->cap, nc = (size_t)ncap;
  int e = 0;
  auto idx = DevBuf<int64_t>::grown(s->act_idx, nc, oc, &e);
  auto w = DevBuf<double>::grown(s->act_w, nc, oc, &e);
  auto norm = DevBuf<double>::grown(s->act_norm, nc, oc, &e);
  auto rows = DevBuf<double>::grown(s->act_rows, nc * d, oc * d, &e);
  if (e) return mem_fail(s, "grow", e);
  s->act_idx = std::move(idx); s->act_w = std::move(w); s->act_norm = std::move(norm); s->act_rows = std::move(rows);
  s->cap = ncap;
  return BCX_OK;
}

int bcx_ensure_gram(bcx_solver* s, int64_t need) {
  if (need <= s->gram_cap) return BCX_OK;
  const int64_t ncap = std::max<int64_t>((need + 63) / 64 * 64, std::max<int64_t>(256, s->gram_cap * 2));
  const size_t oc = (size_t)s->gram_cap, nc = (size_t)ncap;
  int e = 0;
  // gram / hinv change their leading dimension: copied row by row
  auto mat = [&](const DevBuf<double>& m) { return DevBuf<double>::grown_rows(m, oc, nc, nc, oc, &e); };
  auto gram = mat(s->gram), hinv = mat(s->hinv), hinv_lo = mat(s->hinv_lo);
  auto cvec = DevBuf<double>::grown(s->cvec, nc, oc, &e);
  auto plist = DevBuf<int32_t>::grown(s->plist, nc, oc, &e), ppos = DevBuf<int32_t>::grown(s->ppos, nc, oc, &e);
  auto x = DevBuf<double>::grown(s->nn_x, nc, oc, &e);
  // scratch of one step: nothing to keep
  auto z = DevBuf<double>::grown(s->nn_z, nc, 0, &e), wv = DevBuf<double>::grown(s->nn_wv, nc, 0, &e);
  auto tmp = DevBuf<double>::grown(s->nn_tmp, 16 * nc, 0, &e);   // t0..t3 + the exchange ring of grid_lh.h (GRID_RING = 16 buffers)
  auto flag = DevBuf<int32_t>::grown(s->nn_flag, nc, 0, &e);
  auto wbak = DevBuf<double>::grown(s->nn_wbak, nc, 0, &e), xr = DevBuf<double>::grown(s->nn_xr, 2 * nc, 0, &e);
  if (e) return mem_fail(s, "grow", e);
  s->gram = std::move(gram); s->hinv = std::move(hinv); s->hinv_lo = std::move(hinv_lo);
  s->cvec = std::move(cvec); s->plist = std::move(plist); s->ppos = std::move(ppos); s->nn_x = std::move(x);
  s->nn_z = std::move(z); s->nn_wv = std::move(wv); s->nn_tmp = std::move(tmp);
  s->nn_flag = std::move(flag); s->nn_wbak = std::move(wbak); s->nn_xr = std::move(xr);
  s->gram_cap = ncap;
  return BCX_OK;
}

static int ensure_trace(bcx_solver* s, int64_t need) {
  if (need <= s->trace_cap) return BCX_OK;
  const size_t nc = (size_t)std::max<int64_t>(need, 1024);
  int e = 0;
  auto sel = DevBuf<int64_t>::grown(s->tr_sel, nc, 0, &e);
  auto err = DevBuf<double>::grown(s->tr_err, nc, 0, &e);
  auto status = DevBuf<int32_t>::grown(s->tr_status, nc, 0, &e);
  if (e) return mem_fail(s, "grow", e);
  s->tr_sel = std::move(sel); s->tr_err = std::move(err); s->tr_status = std::move(status);
  s->trace_cap = (int64_t)nc;
  return BCX_OK;
}

int bcx_ensure_grid_counter(bcx_solver* s) {
  if (s->grid_counter) return BCX_OK;
  if (s->grid_counter.alloc(BCX_GRID_WORDS, true) != 0) { s->err = "grid counter allocation failed"; return BCX_ERR_NOMEM; }
  return BCX_OK;
}

// ---- build ---------------------------------------------------------------------------------
extern "C" int bcx_build_begin(bcx_solver* s, int64_t itrs, double tol, int32_t* skip) {
  if (!s || !skip) return BCX_ERR_ARG;
  if (!s->finalized) { s->err = "bcx_build_begin: call bcx_finalize first"; return BCX_ERR_STATE; }
  BCX_HIP(hipSetDevice(s->cfg.device));
  *skip = 0;
  DevState h;
  int rc = read_state(s, &h);
  if (rc != BCX_OK) return rc;
  if (h.limit || s->cfg.n_global == 0 || itrs <= 0) { *skip = 1; return BCX_OK; }   // snnls.py:32-38
  s->k_ub = h.k;
  if ((rc = ensure_slots(s, (int64_t)h.k + itrs))) return rc;
  if (s->cfg.alg == BCX_ALG_OMP) {
    if ((rc = bcx_ensure_gram(s, (int64_t)h.k + itrs))) return rc;
    if ((rc = bcx_ensure_grid_counter(s))) return rc;
    BCX_HIP(hipMemsetAsync(s->grid_counter, 0, 2 * sizeof(unsigned long long), s->stream));
    s->grid_epoch = 0;
    s->grid_dirty = false;
  }
  if ((rc = ensure_trace(s, itrs))) return rc;
  return bcx_launch_begin(s, itrs, tol);
}

// Event pairs around the scan launch, on every prof_every-th launch: a pair costs 7-12 us of stream time
// (measured: GIGA N=1M d=256 171 -> 159 us per iteration without them), so the bench samples.
static int prof_begin(bcx_solver* s) {
  if (!s->profile) return BCX_OK;
  s->prof_now = (s->prof_tick++ % s->prof_every) == 0;
  if (!s->prof_now) return BCX_OK;
  if (s->prof_used == s->prof_events.size()) {
    hipEvent_t a, b;
    BCX_HIP(hipEventCreate(&a));
    BCX_HIP(hipEventCreate(&b));
    s->prof_events.emplace_back(a, b);
  }
  BCX_HIP(hipEventRecord(s->prof_events[s->prof_used].first, s->stream));
  return BCX_OK;
}
static int prof_end(bcx_solver* s) {
  if (!s->profile || !s->prof_now) return BCX_OK;
  BCX_HIP(hipEventRecord(s->prof_events[s->prof_used].second, s->stream));
  s->prof_used++;
  return BCX_OK;
}

static int step_scan(bcx_solver* s, void* send_dev, int exact, bool with_tail) {
  if (!s->finalized) { s->err = "solver not finalized"; return BCX_ERR_STATE; }
  double* send = send_dev ? (double*)send_dev : s->rec_local;
  int rc;
  if (exact && (rc = bcx_launch_resume_exact(s))) return rc;
  if ((rc = prof_begin(s))) return rc;
  if ((rc = bcx_launch_scan(s, exact))) return rc;
  if ((rc = prof_end(s))) return rc;
  if (with_tail) return bcx_launch_tail(s, exact);   // resolve + apply in one launch (single shard, GIGA/FW)
  return bcx_launch_resolve(s, send, exact);
}

// the scan of one enqueued iteration: the 4-bit front pass with its second stage + refine (screen4.hip), the 8-bit screen + refine
// (screen8.hip) or the storage-precision / exact scan
static int front_scan(bcx_solver* s, int exact, bool tier, bool four) {
  int rc;
  if (exact && (rc = bcx_launch_resume_exact(s))) return rc;
  if ((rc = prof_begin(s))) return rc;
  if ((rc = (tier && !exact) ? (four ? bcx_launch_screen4(s) : bcx_launch_screen(s)) : bcx_launch_scan(s, exact))) return rc;
  return prof_end(s);
}

// (the host-driven step always takes the storage-precision scan: the tier's redo lives in bcx_build_poll's enqueue route)
extern "C" int bcx_step_scan(bcx_solver* s, void* send_dev) { if (s) s->scr_batch = false; return s ? step_scan(s, send_dev, 0, false) : BCX_ERR_ARG; }
extern "C" int bcx_step_scan_exact(bcx_solver* s, void* send_dev) { if (s) s->scr_batch = false; return s ? step_scan(s, send_dev, 1, false) : BCX_ERR_ARG; }

extern "C" int bcx_step_apply(bcx_solver* s, const void* recv_dev) {
  if (!s) return BCX_ERR_ARG;
  return bcx_launch_apply(s, recv_dev ? (const double*)recv_dev : s->rec_local);
}

// one whole iteration without the host: single shard, or row shards with an attached peer mailbox
static int enqueue_one_launch(bcx_solver* s, int exact, bool tier, bool four) {
  if (!s->finalized) { s->err = "solver not finalized"; return BCX_ERR_STATE; }
  int rc;
  if (s->cfg.world_size != 1) {
    if (!s->exchange_ready) {
      s->err = "bcx_build_enqueue on a row shard needs bcx_exchange_attach (or drive bcx_step_scan / bcx_step_apply)";
      return BCX_ERR_ARG;
    }
    if ((rc = front_scan(s, exact, tier, false))) return rc;
    return bcx_launch_tail_exchange(s, exact);
  }
  if ((rc = front_scan(s, exact, tier, four))) return rc;
  if (s->cfg.alg == BCX_ALG_OMP) {
    // scan, then the fused resolve + OMP step (omp_lh.hip); where that does not apply: resolve_kernel + the multi-kernel step
    rc = bcx_launch_omp_fused(s, exact);
    if (rc != 1) return rc;
    if ((rc = bcx_launch_resolve(s, s->rec_local, exact))) return rc;
    return bcx_launch_apply(s, s->rec_local);
  }
  return bcx_launch_tail(s, exact);   // resolve + apply in one launch (single shard, GIGA/FW)
}

static int enqueue_one(bcx_solver* s, int exact, bool tier, bool four = false) {
  const int rc = enqueue_one_launch(s, exact, tier, four);
  if (rc == BCX_OK) s->enq_unpolled = true;   // until bcx_build_poll (or bcx_reset): bcx_screen4_probe refuses meanwhile
  return rc;
}

// `itrs` iterations through the 8-bit tier when it is on (default), else as the parent did
static int enqueue_many(bcx_solver* s, int64_t itrs) {
  int rc = bcx_screen_build(s);
  if (rc != BCX_OK) return rc;
  const bool tier = bcx_screen_on(s) && s->scr_valid;
  if (tier && (rc = bcx_screen4_build(s))) return rc;
  const bool tier4 = tier && bcx_screen4_on(s) && s->s4_valid;
  s->scr_batch = false;
  for (int64_t i = 0; i < itrs; ++i) {
    s->scr_batch = tier;
    // The 4-bit front pass needs sentinel rows: those the refine kernel of the tier iteration enqueued just before left.  s4_warm counts the
    // plain 8-bit iterations still due: two after finalize / reset / a reload (the second query after a fresh start is still
    // far from the first), one after a redone iteration.  Decided here, without a device round trip.
    const bool four = tier4 && s->s4_warm == 0;
    rc = enqueue_one(s, 0, tier, four);
    if (rc != BCX_OK) return rc;
    if (tier && s->s4_warm > 0) s->s4_warm -= 1;
  }
  return BCX_OK;
}

extern "C" int bcx_build_enqueue(bcx_solver* s, int64_t itrs) {
  if (!s) return BCX_ERR_ARG;
  if (!s->finalized) { s->err = "solver not finalized"; return BCX_ERR_STATE; }
  return enqueue_many(s, itrs);
}

extern "C" int bcx_build_enqueue_exact(bcx_solver* s) {
  if (!s) return BCX_ERR_ARG;
  if (!s->finalized) { s->err = "solver not finalized"; return BCX_ERR_STATE; }
  s->scr_batch = false;
  return enqueue_one(s, 1, false);
}

// ---- peer mailbox --------------------------------------------------------------------------------
static int mailbox_alloc(bcx_solver* s) {
  if (s->mbox) return BCX_OK;
  const int world = s->cfg.world_size;
  const size_t bytes = bcx_mailbox_slot_offset(world) + 2 * (size_t)world * (s->cfg.d + BCX_REC_HDR) * sizeof(double);
  // fine-grained: stores from peer GPUs become visible to a kernel that is already running here
  const int e = s->mbox.alloc(bytes, false, true);
  if (e != 0) {
    (void)hipGetLastError();
    s->err = std::string("peer mailbox: fine-grained allocation failed: ") + hipGetErrorString((hipError_t)e);
    return BCX_ERR_HIP;
  }
  BCX_HIP(hipMemset(s->mbox, 0, bytes));
  BCX_HIP(hipDeviceSynchronize());
  return BCX_OK;
}

extern "C" int bcx_exchange_export(bcx_solver* s, void* handle_out, int32_t handle_bytes) {
  if (!s || !handle_out) return BCX_ERR_ARG;
  if (handle_bytes < (int32_t)sizeof(hipIpcMemHandle_t)) { s->err = "bcx_exchange_export: handle buffer too small"; return BCX_ERR_ARG; }
  if ((size_t)s->cfg.d * sizeof(double) > 144 * 1024) {
    // the exchange kernels stage one record (d doubles) in LDS; longer rows use the host-driven all-gather exchange
    s->err = "peer mailbox: rows of more than 18432 values exchange their records through the all-gather";
    return BCX_ERR_ARG;
  }
  BCX_HIP(hipSetDevice(s->cfg.device));
  int rc = mailbox_alloc(s);
  if (rc != BCX_OK) return rc;
  hipIpcMemHandle_t h;
  BCX_HIP(hipIpcGetMemHandle(&h, s->mbox));
  memset(handle_out, 0, handle_bytes);
  memcpy(handle_out, &h, sizeof(h));
  return BCX_OK;
}

extern "C" int bcx_exchange_attach(bcx_solver* s, const void* handles, int32_t handle_bytes, double timeout_s) {
  if (!s || !handles) return BCX_ERR_ARG;
  if (s->exchange_ready) return BCX_OK;
  if (!s->mbox) { s->err = "bcx_exchange_attach: call bcx_exchange_export first"; return BCX_ERR_STATE; }
  if (handle_bytes < (int32_t)sizeof(hipIpcMemHandle_t)) return BCX_ERR_ARG;
  BCX_HIP(hipSetDevice(s->cfg.device));
  const int world = s->cfg.world_size;
  if (world > BCX_APPLY_THREADS) { s->err = "peer mailbox supports at most 256 shards"; return BCX_ERR_ARG; }
  if (!s->peer_mbox.empty()) {
    // attached before and disabled since: the earlier attachment goes first (nothing enqueued may still be reading it)
    BCX_HIP(hipStreamSynchronize(s->stream));
    s->close_peers();
    s->peer_tab.reset(); s->xseq.reset(); s->xprobe.reset(); s->rec_gather.reset();
  }
  // everything is built in locals and handed to the solver at the end: a failure on the way leaves nothing mapped
  std::vector<void*> peers(world, nullptr);
  auto unmap = [&]() {
    for (int v = 0; v < world; ++v)
      if (v != s->cfg.rank && peers[v]) (void)hipIpcCloseMemHandle(peers[v]);
  };
  for (int w = 0; w < world; ++w) {
    if (w == s->cfg.rank) { peers[w] = s->mbox; continue; }
    hipIpcMemHandle_t h;
    memcpy(&h, (const char*)handles + (size_t)w * handle_bytes, sizeof(h));
    hipError_t e = hipIpcOpenMemHandle(&peers[w], h, hipIpcMemLazyEnablePeerAccess);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      peers[w] = nullptr;
      s->err = "peer mailbox: cannot map shard " + std::to_string(w) + ": " + hipGetErrorString(e);
      unmap();
      return BCX_ERR_HIP;
    }
  }
  DevBuf<void*> tab;
  DevBuf<unsigned long long> xseq;
  DevBuf<int32_t> xprobe;
  DevBuf<double> gather;
  int e;
  if ((e = tab.alloc((size_t)world, true)) || (e = xseq.alloc(8, true)) || (e = xprobe.alloc(1, true)) ||
      (e = gather.alloc((size_t)world * (s->cfg.d + BCX_REC_HDR), true))) {
    s->err = std::string("peer mailbox: ") + hipGetErrorString((hipError_t)e);
    unmap();
    return BCX_ERR_NOMEM;
  }
  const hipError_t ec = hipMemcpy(tab, peers.data(), (size_t)world * sizeof(void*), hipMemcpyHostToDevice);
  if (ec != hipSuccess) { unmap(); return mem_fail(s, "peer mailbox: hipMemcpy", (int)ec); }
  s->peer_mbox = std::move(peers);
  s->peer_tab = std::move(tab); s->xseq = std::move(xseq); s->xprobe = std::move(xprobe); s->rec_gather = std::move(gather);
  if (timeout_s > 0.0) s->exchange_timeout_s = timeout_s;
  s->exchange_ready = true;
  return BCX_OK;
}

extern "C" int bcx_exchange_probe(bcx_solver* s, int32_t* result) {
  if (!s || !result) return BCX_ERR_ARG;
  if (!s->exchange_ready) { s->err = "bcx_exchange_probe: no peer mailbox attached"; return BCX_ERR_STATE; }
  BCX_HIP(hipSetDevice(s->cfg.device));
  int rc = bcx_launch_exchange_probe(s);
  if (rc != BCX_OK) return rc;
  BCX_HIP(hipStreamSynchronize(s->stream));
  BCX_HIP(hipMemcpy(result, s->xprobe, sizeof(int32_t), hipMemcpyDeviceToHost));
  return BCX_OK;
}

extern "C" int bcx_exchange_set_timeout(bcx_solver* s, double timeout_s) {
  if (!s || !(timeout_s > 0.0)) return BCX_ERR_ARG;
  s->exchange_timeout_s = timeout_s;
  return BCX_OK;
}

// Device-side timing of the record exchange since the last reset: n exchanges, mean / max (microseconds) of the wait for
// the slowest peer's record after this shard posted its own, and of the whole exchange step.
extern "C" int bcx_exchange_stats(bcx_solver* s, int64_t* n, double* wait_us_mean, double* wait_us_max, double* total_us_mean,
                                  double* total_us_max, int32_t reset) {
  if (!s) return BCX_ERR_ARG;
  unsigned long long h[5] = {0, 0, 0, 0, 0};
  if (s->xseq) {
    BCX_HIP(hipSetDevice(s->cfg.device));
    BCX_HIP(hipStreamSynchronize(s->stream));
    BCX_HIP(hipMemcpy(h, s->xseq + 1, sizeof h, hipMemcpyDeviceToHost));
    if (reset) BCX_HIP(hipMemset(s->xseq + 1, 0, sizeof h));
  }
  const double per = h[0] ? 1.0 / (double)h[0] : 0.0, us = 1.0 / 100.0;   // wall_clock64: 100 MHz
  if (n) *n = (int64_t)h[0];
  if (wait_us_mean) *wait_us_mean = (double)h[1] * per * us;
  if (wait_us_max) *wait_us_max = (double)h[2] * us;
  if (total_us_mean) *total_us_mean = (double)h[3] * per * us;
  if (total_us_max) *total_us_max = (double)h[4] * us;
  return BCX_OK;
}

extern "C" int bcx_exchange_disable(bcx_solver* s) {
  if (!s) return BCX_ERR_ARG;
  s->exchange_ready = false;   // mappings stay until bcx_destroy; the host-driven step_scan / step_apply path is used again
  return BCX_OK;
}

extern "C" int bcx_build_poll(bcx_solver* s, int64_t* n_done, int32_t* need_exact, int32_t* limit) {
  if (!s) return BCX_ERR_ARG;
  DevState h;
  int rc = read_state(s, &h);
  if (rc != BCX_OK) return rc;
  // A tier iteration that halted (its capture overflowed, or the survivors overflowed resolve_core's window) is redone HERE
  // with the storage-precision scan -- one scan of the stored rows, not the fp64 exact scan, and not an exact fallback --
  // and the rest of the call is enqueued again behind it.  The halt is replicated state, so every rank of a row-sharded
  // build takes the same route.  Only a halt of the storage-precision iteration itself is reported as need_exact.
  // Drop rule: 4 such halts within 256 screened iterations (far above the < 1 % the tier is built for: rows of low
  // numerical rank, near-duplicates, GIGA past M > d) drop the tier until bcx_reset; a step then costs what it did without it.
  while (h.halt == HALT_NEED_EXACT && s->scr_batch && s->scr_stat) {
    unsigned long long st8[SCR_WORDS];
    BCX_HIP(hipMemcpy(st8, s->scr_stat, sizeof st8, hipMemcpyDeviceToHost));
    if (!st8[SCR_ARMED]) break;                       // the storage-precision redo itself halted
    if (st8[SCR4_LAST] != 0) {
      // the halted iteration went through the 4-bit front pass (a full list segment, or a capture overflow behind it): the
      // same rule on the 4-bit tier's own count drops the solver to the 8-bit tier, never straight to the storage scan
      s->s4_halts += 1;
      for (int i = 3; i > 0; --i) s->s4_ovf_at[i] = s->s4_ovf_at[i - 1];
      s->s4_ovf_at[0] = st8[SCR4_ITERS];
      s->s4_redos += 1;
      if (s->s4_halts >= 4 && s->s4_ovf_at[0] - s->s4_ovf_at[3] < 256 && !s->s4_dropped) { s->s4_dropped = 1; s->s4_drops += 1; }
    } else {
      s->scr_halts += 1;
      for (int i = 3; i > 0; --i) s->scr_ovf_at[i] = s->scr_ovf_at[i - 1];
      s->scr_ovf_at[0] = st8[SCR_ITERS];
      if (s->scr_halts >= 4 && s->scr_ovf_at[0] - s->scr_ovf_at[3] < 256) s->scr_dropped = 1;
    }
    if (s->s4_warm < 1) s->s4_warm = 1;                // the redo writes no tier partials: one plain 8-bit iteration first
    if ((rc = bcx_launch_resume_store(s))) return rc;
    if ((rc = enqueue_one(s, 0, false))) return rc;
    const int64_t rest = h.itrs - h.it - 1;
    if (rest > 0 && (rc = enqueue_many(s, rest))) return rc;
    else if (rest <= 0) s->scr_batch = false;
    if ((rc = read_state(s, &h))) return rc;
  }
  s->enq_unpolled = false;
  if (h.halt == HALT_GRID_TIMEOUT) { s->err = "OMP step: grid barrier timed out"; return BCX_ERR_STATE; }
  if (h.halt == HALT_EXCHANGE_TIMEOUT) {
    // which peers' flags never arrived (recorded by the waiting lanes, csrc/resolve.hip mailbox_exchange)
    unsigned long long late[2] = {0, 0};
    std::string who;
    if (s->xseq && hipMemcpy(late, s->xseq + 6, sizeof late, hipMemcpyDeviceToHost) == hipSuccess) {
      for (int r = 0; r < s->cfg.world_size && r < 64; ++r)
        if (late[0] >> r & 1ull) who += (who.empty() ? "" : ", ") + std::to_string(r);
      (void)hipMemset(s->xseq + 6, 0, sizeof late);
    } else (void)hipGetLastError();
    s->err = "peer mailbox: rank " + std::to_string(s->cfg.rank) + " got no record from rank(s) " + (who.empty() ? "?" : who) +
             " within " + std::to_string(s->exchange_timeout_s) + " s (exchange #" + std::to_string(late[1]) + ")";
    return BCX_ERR_EXCHANGE;
  }
  if (n_done) *n_done = h.it;
  if (need_exact) *need_exact = (h.halt == HALT_NEED_EXACT);
  if (limit) *limit = h.limit;
  if (s->profile) {
    // launches issued after the state machine stopped (end of call, latch) return at once: keep only launches that
    // did the scan -- one that "read" the shard faster than 1.5x the HBM peak cannot have (a whole batch may consist
    // of such launches, e.g. everything enqueued after a latch, so the test is absolute, not relative to the batch)
    // (with the 8-bit tier on, a launch reads one byte per element)
    // (half a byte with the 4-bit front pass)
    const bool on8 = bcx_screen_on(s) && s->scr_valid;
    const double min_ms = (double)s->cfg.n_local * s->cfg.d * (on8 ? ((bcx_screen4_on(s) && s->s4_valid) ? 0.5 : 1.0) : (double)s->elem) / 12.0e9;
    for (size_t i = 0; i < s->prof_used; ++i) {
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, s->prof_events[i].first, s->prof_events[i].second) != hipSuccess) continue;
      if ((double)ms >= min_ms) { s->prof_ms += ms; s->prof_launches += 1; }
    }
    s->prof_used = 0;
  }
  return BCX_OK;
}

extern "C" int bcx_build_trace(bcx_solver* s, int64_t* sel, double* err, int32_t* status, int64_t cap, int64_t* n_out) {
  if (!s) return BCX_ERR_ARG;
  DevState h;
  int rc = read_state(s, &h);
  if (rc != BCX_OK) return rc;
  const int64_t n = std::min<int64_t>(h.it, cap);
  if (n > 0) {
    if (sel) BCX_HIP(hipMemcpy(sel, s->tr_sel, (size_t)n * 8, hipMemcpyDeviceToHost));
    if (err) BCX_HIP(hipMemcpy(err, s->tr_err, (size_t)n * 8, hipMemcpyDeviceToHost));
    if (status) BCX_HIP(hipMemcpy(status, s->tr_status, (size_t)n * 4, hipMemcpyDeviceToHost));
  }
  if (n_out) *n_out = n;
  return BCX_OK;
}

// ---- read-out ------------------------------------------------------------------------------
extern "C" int bcx_active_count(bcx_solver* s, int64_t* k) {
  if (!s || !k) return BCX_ERR_ARG;
  DevState h;
  int rc = read_state(s, &h);
  if (rc != BCX_OK) return rc;
  *k = h.k;
  return BCX_OK;
}

extern "C" int bcx_get_weights(bcx_solver* s, int64_t* idx, double* w, int64_t cap, int64_t* k) {
  if (!s || !k) return BCX_ERR_ARG;
  DevState h;
  int rc = read_state(s, &h);
  if (rc != BCX_OK) return rc;
  const int64_t n = std::min<int64_t>(h.k, cap);
  if (n > 0) {
    if (idx) BCX_HIP(hipMemcpy(idx, s->act_idx, (size_t)n * 8, hipMemcpyDeviceToHost));
    if (w) BCX_HIP(hipMemcpy(w, s->act_w, (size_t)n * 8, hipMemcpyDeviceToHost));
  }
  *k = h.k;
  return BCX_OK;
}

extern "C" int bcx_error(bcx_solver* s, double* err) {
  if (!s || !err) return BCX_ERR_ARG;
  if (!s->finalized) { s->err = "solver not finalized"; return BCX_ERR_STATE; }
  int rc = bcx_launch_error_refresh(s);
  if (rc != BCX_OK) return rc;
  DevState h;
  if ((rc = read_state(s, &h))) return rc;
  *err = h.err;
  return BCX_OK;
}

extern "C" int bcx_reached_numeric_limit(bcx_solver* s, int32_t* limit) {
  if (!s || !limit) return BCX_ERR_ARG;
  DevState h;
  int rc = read_state(s, &h);
  if (rc != BCX_OK) return rc;
  *limit = h.limit;
  return BCX_OK;
}

extern "C" int bcx_reset(bcx_solver* s) {
  if (!s) return BCX_ERR_ARG;
  if (!s->finalized) return BCX_OK;
  // w = 0, reached_numeric_limit = False (snnls.py:18-20); b, norms and the matrix stay
  DevState h;
  int rc = read_state(s, &h);
  if (rc != BCX_OK) return rc;
  h.k = 0; h.np = 0; h.hvalid = 1; h.omp_ill = 0; h.limit = 0; h.retried = 0; h.active = 0; h.halt = HALT_NONE; h.since_refresh = 0; h.exact_mode = 0;
  h.err = h.bnorm; h.nw = 1.0; h.it = 0; h.itrs = 0;
  BCX_HIP(hipMemcpy(s->st, &h, sizeof h, hipMemcpyHostToDevice));
  BCX_HIP(hipMemset(s->xw, 0, (size_t)s->cfg.d * 8));
  if (s->scr_dropped == 1) s->scr_dropped = 0;      // the overflow rule's drop lasts until here
  s->scr_halts = 0;
  for (int i = 0; i < 4; ++i) s->scr_ovf_at[i] = 0;
  if (s->s4_dropped == 1) s->s4_dropped = 0;
  s->s4_halts = 0;
  for (int i = 0; i < 4; ++i) s->s4_ovf_at[i] = 0;
  s->s4_warm = 2;                                   // a fresh start: the first queries are far from the last ones
  s->enq_unpolled = false;                          // (read_state above waited for whatever was enqueued)
  // error() with an empty list must give ||b|| computed the same way as after finalize
  return bcx_launch_error_refresh(s);
}

extern "C" int bcx_set_check_monotone(bcx_solver* s, int32_t on) {
  if (!s) return BCX_ERR_ARG;
  BCX_HIP(hipSetDevice(s->cfg.device));
  DevState h;
  int rc = read_state(s, &h);
  if (rc != BCX_OK) return rc;
  h.no_monotone = on ? 0 : 1;
  BCX_HIP(hipMemcpy(s->st, &h, sizeof h, hipMemcpyHostToDevice));
  return BCX_OK;
}

extern "C" int bcx_optimize(bcx_solver* s, double tol, int32_t* accepted) {
  if (!s || !accepted) return BCX_ERR_ARG;
  if (!s->finalized) { s->err = "solver not finalized"; return BCX_ERR_STATE; }
  DevState h;
  int rc = read_state(s, &h);
  if (rc != BCX_OK) return rc;
  if ((rc = ensure_slots(s, std::max<int64_t>(h.k, 1)))) return rc;
  if ((rc = bcx_ensure_gram(s, std::max<int64_t>(h.k, 1)))) return rc;
  if ((rc = bcx_launch_optimize(s, tol))) return rc;
  DevState h2;
  if ((rc = read_state(s, &h2))) return rc;
  if (h2.halt == HALT_GRID_TIMEOUT) { s->err = "optimize: grid barrier timed out"; return BCX_ERR_STATE; }
  *accepted = h2.limit ? 0 : 1;
  return BCX_OK;
}

// ---- introspection / measurement ---------------------------------------------------------------
extern "C" int bcx_get_vector(bcx_solver* s, int32_t which, double* out) {
  if (!s || !out) return BCX_ERR_ARG;
  const double* src = nullptr;
  switch (which) {
    case 0: src = s->b; break;
    case 1: src = s->xw; break;
    case 2: src = s->q64; break;
    case 3: src = s->q64 + s->ld64; break;
    default: return BCX_ERR_ARG;
  }
  BCX_HIP(hipStreamSynchronize(s->stream));
  BCX_HIP(hipMemcpy(out, src, (size_t)s->cfg.d * 8, hipMemcpyDeviceToHost));
  return BCX_OK;
}

extern "C" int bcx_get_norms(bcx_solver* s, int64_t begin, int64_t count, double* out) {
  if (!s || !out || begin < 0 || begin + count > s->cfg.n_local) return BCX_ERR_ARG;
  BCX_HIP(hipStreamSynchronize(s->stream));
  BCX_HIP(hipMemcpy(out, s->norms + begin, (size_t)count * 8, hipMemcpyDeviceToHost));
  return BCX_OK;
}

// The stored (normalised) rows [begin, begin + count) as the scan reads them: count x ld elements of the storage type
// (ld = d rounded up to 16 bytes' worth of elements, returned in *ld_out; elements beyond d are padding).
extern "C" int bcx_get_stored_rows(bcx_solver* s, int64_t begin, int64_t count, void* out, int32_t* ld_out) {
  if (!s || begin < 0 || count < 0 || begin + count > s->cfg.n_local) return BCX_ERR_ARG;
  if (ld_out) *ld_out = s->ld;
  if (count == 0) return BCX_OK;
  if (!out) return BCX_ERR_ARG;
  BCX_HIP(hipSetDevice(s->cfg.device));
  BCX_HIP(hipStreamSynchronize(s->stream));
  BCX_HIP(hipMemcpy(out, (const char*)s->An + (size_t)begin * s->ld * s->elem, (size_t)count * s->ld * s->elem, hipMemcpyDeviceToHost));
  return BCX_OK;
}

extern "C" int bcx_time_scan(bcx_solver* s, int32_t reps, int32_t exact, double* ms_per_launch, double* bytes_per_launch) {
  if (!s || reps < 1) return BCX_ERR_ARG;
  if (!s->finalized) { s->err = "solver not finalized"; return BCX_ERR_STATE; }
  BCX_HIP(hipSetDevice(s->cfg.device));
  // the scan only runs while the state machine is active: force it for the measurement
  DevState h;
  int rc = read_state(s, &h);
  if (rc != BCX_OK) return rc;
  DevState forced = h;
  forced.active = 1;
  BCX_HIP(hipMemcpy(s->st, &forced, sizeof forced, hipMemcpyHostToDevice));
  hipEvent_t e0, e1;
  BCX_HIP(hipEventCreate(&e0));
  BCX_HIP(hipEventCreate(&e1));
  for (int i = 0; i < 3 && rc == BCX_OK; ++i) rc = bcx_launch_scan(s, exact);
  if (rc == BCX_OK) (void)hipEventRecord(e0, s->stream);
  for (int i = 0; i < reps && rc == BCX_OK; ++i) rc = bcx_launch_scan(s, exact);
  if (rc != BCX_OK) {
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    (void)hipMemcpy(s->st, &h, sizeof h, hipMemcpyHostToDevice);
    return rc;
  }
  BCX_HIP(hipEventRecord(e1, s->stream));
  BCX_HIP(hipEventSynchronize(e1));
  float ms = 0.f;
  BCX_HIP(hipEventElapsedTime(&ms, e0, e1));
  BCX_HIP(hipEventDestroy(e0));
  BCX_HIP(hipEventDestroy(e1));
  BCX_HIP(hipMemcpy(s->st, &h, sizeof h, hipMemcpyHostToDevice));
  if (ms_per_launch) *ms_per_launch = (double)ms / reps;
  const bool raw64 = exact && s->cfg.store_dtype != BCX_F64 && s->A64;
  if (bytes_per_launch) *bytes_per_launch = (double)s->cfg.n_local * s->cfg.d * (raw64 ? 8.0 : (double)s->elem);
  return BCX_OK;
}

// A caller's query for one scan (bcx_argmax_correlation, bcx_screen4_probe): the storage-precision query of the scan, with the
// fp64 query of the re-score when `with64`; *qn_out / *E_out are DevState's qscale / qexp for it.
static int upload_query(bcx_solver* s, const double* query_host, bool with64, double* qn_out, int* E_out) {
  const int d = s->cfg.d;
  std::vector<double> q64((size_t)s->ld64, 0.0);
  // |q| without leaving fp64's range at any scale of q: the squares are taken of q * 2^-E0, E0 the exponent of the largest
  // element; the fp32 query then holds q * 2^-E with E the exponent of |q| (apply_common.h store_query: same rule)
  double qmax = 0.0;
  for (int j = 0; j < d; ++j) { q64[j] = query_host[j]; qmax = std::fmax(qmax, std::fabs(query_host[j])); }
  const bool scalable = qmax > 0.0 && qmax < INFINITY;     // (a zero, infinite or NaN query is scanned as it is)
  const int E0 = scalable ? std::ilogb(qmax) : 0;
  double qn = 0.0;
  for (int j = 0; j < d; ++j) { const double t = std::ldexp(query_host[j], -E0); qn += t * t; }
  qn = std::sqrt(qn);                                      // |q| * 2^-E0, in [1, 2 sqrt(d))
  int E = 0;
  if (with64) BCX_HIP(hipMemcpy(s->q64, q64.data(), (size_t)s->ld64 * 8, hipMemcpyHostToDevice));
  if (s->cfg.store_dtype == BCX_F64) {
    std::vector<double> qs((size_t)s->ld, 0.0);
    for (int j = 0; j < d; ++j) qs[j] = query_host[j];
    BCX_HIP(hipMemcpy(s->qst, qs.data(), (size_t)s->ld * 8, hipMemcpyHostToDevice));
    qn = std::ldexp(qn, E0);                               // (not read: the fp64 scan's error term is zero)
  } else {
    const int E1 = (scalable && qn > 0.0 && qn < INFINITY) ? std::ilogb(qn) : 0;   // (a NaN element: no second step)
    E = E0 + E1;
    std::vector<float> qs((size_t)s->ld, 0.f);
    for (int j = 0; j < d; ++j) qs[j] = (float)std::ldexp(query_host[j], -E);
    BCX_HIP(hipMemcpy(s->qst, qs.data(), (size_t)s->ld * 4, hipMemcpyHostToDevice));
    qn = std::ldexp(qn, -E1);
  }
  *qn_out = qn; *E_out = E;
  return BCX_OK;
}

// One N-way correlation scan with a caller-supplied query: arg-max_n An[n] . q (first maximum) and the
// exact fp64 score.  This is the select step of SparseVI on already projected vectors
// (sparsevi.py:49-56: corrs = vecs.dot(resid)/||vecs||/S, argmax).  Single-query algorithms only.
extern "C" int bcx_argmax_correlation(bcx_solver* s, const double* query_host, int64_t* idx, double* score) {
  if (!s || !query_host || !idx || !score) return BCX_ERR_ARG;
  if (!s->finalized) { s->err = "solver not finalized"; return BCX_ERR_STATE; }
  if (s->cfg.alg == BCX_ALG_GIGA) { s->err = "bcx_argmax_correlation needs a single-query solver (FW/OMP)"; return BCX_ERR_ARG; }
  BCX_HIP(hipSetDevice(s->cfg.device));
  DevState h;
  int rc = read_state(s, &h);
  if (rc != BCX_OK) return rc;
  double qn = 0.0;
  int E = 0;
  if ((rc = upload_query(s, query_host, true, &qn, &E))) return rc;
  DevState forced = h;
  forced.active = 1; forced.exact_mode = 0; forced.qscale = qn; forced.qexp = E;
  double rec[BCX_REC_HDR];
  for (int attempt = 0; attempt < 2; ++attempt) {
    forced.exact_mode = attempt;
    BCX_HIP(hipMemcpy(s->st, &forced, sizeof forced, hipMemcpyHostToDevice));
    if ((rc = bcx_launch_scan(s, attempt))) return rc;
    if ((rc = bcx_launch_resolve(s, s->rec_local, attempt))) return rc;
    BCX_HIP(hipStreamSynchronize(s->stream));
    BCX_HIP(hipMemcpy(rec, s->rec_local, sizeof rec, hipMemcpyDeviceToHost));
    if (rec[3] != BCX_REC_OVERFLOW) break;
  }
  BCX_HIP(hipMemcpy(s->st, &h, sizeof h, hipMemcpyHostToDevice));
  if (rec[3] != BCX_REC_VALID) { s->err = "no rows to scan"; return BCX_ERR_STATE; }
  *idx = (int64_t)rec[1];
  *score = rec[0];
  return BCX_OK;
}

extern "C" int bcx_stats(bcx_solver* s, int64_t* exact_fallbacks, int64_t* candidates, int64_t* resolves) {
  if (!s) return BCX_ERR_ARG;
  DevState h;
  int rc = read_state(s, &h);
  if (rc != BCX_OK) return rc;
  if (exact_fallbacks) *exact_fallbacks = h.n_exact;
  if (candidates) *candidates = h.n_cand;
  if (resolves) *resolves = h.n_resolved;
  return BCX_OK;
}

// The 8-bit screening tier (screen8.hip) since construction: out8 = {1 if the next enqueued iteration goes through it,
// iterations screened, survivors re-scored from the stored rows (over the iterations that did not overflow), capture
// overflows, iterations redone with the storage-precision scan (capture overflows + survivor storms in resolve), drop state
// (0 in use, 1 dropped by the overflow rule until bcx_reset, 2 no memory for the shadow, 3 switched off or not applicable),
// bytes of device memory the tier holds, microseconds the last build of the shadow took}
extern "C" int bcx_screen_stats(bcx_solver* s, int64_t* out8) {
  if (!s || !out8) return BCX_ERR_ARG;
  unsigned long long st8[SCR_WORDS] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (s->scr_stat) {
    BCX_HIP(hipSetDevice(s->cfg.device));
    BCX_HIP(hipStreamSynchronize(s->stream));
    BCX_HIP(hipMemcpy(st8, s->scr_stat, sizeof st8, hipMemcpyDeviceToHost));
  }
  const bool possible = s->scr_enabled && s->cfg.store_dtype != BCX_F64 && s->cfg.d <= 4096 && s->cfg.n_local > 0;
  out8[0] = bcx_screen_on(s) ? 1 : 0;
  out8[1] = (int64_t)st8[SCR_ITERS];
  out8[2] = (int64_t)st8[SCR_SURVIVORS];
  out8[3] = (int64_t)st8[SCR_OVERFLOWS];
  out8[4] = (int64_t)st8[SCR_REDOS];
  out8[5] = !possible ? 3 : s->scr_dropped;
  out8[6] = s->Aq ? (int64_t)s->scr_sb.count() * (s->ld8 + 8) + (int64_t)BCX_MAX_PARTIALS * BCX_PARTIAL_BYTES + SCR_WORDS * 8 : 0;
  out8[7] = (int64_t)(s->scr_build_ms * 1e3f);
  return BCX_OK;
}

// The 4-bit front pass (screen4.hip) since construction: out8 = {1 if iterations enqueued next go through it once sentinel
// rows exist, 4-bit iterations, rows listed for the second stage, list segments that were full, halted 4-bit iterations
// that were redone, state (0 in use, 1 dropped to the 8-bit tier until bcx_reset, 2 no device memory for the second shadow,
// 3 switched off or not applicable), device bytes of the second shadow and its list, times the drop rule fired}.
extern "C" int bcx_screen4_stats(bcx_solver* s, int64_t* out8) {
  if (!s || !out8) return BCX_ERR_ARG;
  unsigned long long st8[SCR_WORDS];
  for (auto& w : st8) w = 0;
  if (s->scr_stat) {
    BCX_HIP(hipSetDevice(s->cfg.device));
    BCX_HIP(hipStreamSynchronize(s->stream));
    BCX_HIP(hipMemcpy(st8, s->scr_stat, sizeof st8, hipMemcpyDeviceToHost));
  }
  const bool possible = s->s4_enabled && s->scr_enabled && s->cfg.store_dtype != BCX_F64 && s->cfg.d <= 4096 && s->cfg.n_local > 0 &&
                        s->cfg.alg != BCX_ALG_GIGA && s->cfg.world_size == 1;
  out8[0] = bcx_screen4_on(s) ? 1 : 0;
  out8[1] = (int64_t)st8[SCR4_ITERS];
  out8[2] = (int64_t)st8[SCR4_LISTED];
  out8[3] = (int64_t)st8[SCR4_OVERFLOWS];
  out8[4] = s->s4_redos;
  out8[5] = !possible ? 3 : s->s4_dropped;
  out8[6] = s->A4 ? (int64_t)s->s4_sb.count() * (s->ld4 + 8) + (int64_t)BCX_MAX_PARTIALS * (BCX_S4_SEG_CAP + 1) * 4 : 0;
  out8[7] = s->s4_drops;
  return BCX_OK;
}

// Read back `count` rows of the shadow from local row `begin`: codes (count x ld8 bytes, ld8 = d rounded up to 16; returned
// in *ld8_out), scales and bounds (count floats each).  Builds the shadow first if it is due.  BCX_ERR_STATE without a tier.
extern "C" int bcx_screen_read(bcx_solver* s, int64_t begin, int64_t count, void* codes, float* scales, float* bounds, int32_t* ld8_out) {
  if (!s || begin < 0 || count < 0 || begin + count > s->cfg.n_local) return BCX_ERR_ARG;
  if (!s->finalized) { s->err = "solver not finalized"; return BCX_ERR_STATE; }
  BCX_HIP(hipSetDevice(s->cfg.device));
  int rc = bcx_screen_build(s);
  if (rc != BCX_OK) return rc;
  if (!bcx_screen_on(s) || !s->scr_valid) { s->err = "bcx_screen_read: the 8-bit tier is not in use"; return BCX_ERR_STATE; }
  BCX_HIP(hipStreamSynchronize(s->stream));
  if (ld8_out) *ld8_out = s->ld8;
  if (count == 0) return BCX_OK;
  if (codes) BCX_HIP(hipMemcpy(codes, (const char*)s->Aq + (size_t)begin * s->ld8, (size_t)count * s->ld8, hipMemcpyDeviceToHost));
  std::vector<float> sb((size_t)count * 2);
  BCX_HIP(hipMemcpy(sb.data(), s->scr_sb + begin, (size_t)count * 8, hipMemcpyDeviceToHost));
  for (int64_t i = 0; i < count; ++i) {
    if (scales) scales[i] = sb[2 * i];
    if (bounds) bounds[i] = sb[2 * i + 1];
  }
  return BCX_OK;
}

// Both shadows, built if they are due; BCX_ERR_STATE where the 4-bit front pass does not apply (GIGA, fp64 storage, row shards,
// switched off, no memory).
static int screen4_ready(bcx_solver* s, const char* who) {
  if (!s->finalized) { s->err = "solver not finalized"; return BCX_ERR_STATE; }
  BCX_HIP(hipSetDevice(s->cfg.device));
  int rc = bcx_screen_build(s);
  if (rc != BCX_OK) return rc;
  if (bcx_screen_on(s) && s->scr_valid && (rc = bcx_screen4_build(s))) return rc;
  if (!bcx_screen_on(s) || !s->scr_valid || !bcx_screen4_on(s) || !s->s4_valid) {
    s->err = std::string(who) + ": the 4-bit front pass is not in use";
    return BCX_ERR_STATE;
  }
  return BCX_OK;
}

// The twin of bcx_screen_read for the 4-bit shadow: codes (count x ld4 bytes, ld4 = ceil(d / 32) * 16; returned in *ld4_out),
// scale4 and bound4 (count floats each).
extern "C" int bcx_screen4_read(bcx_solver* s, int64_t begin, int64_t count, void* codes, float* scales, float* bounds, int32_t* ld4_out) {
  if (!s || begin < 0 || count < 0 || begin + count > s->cfg.n_local) return BCX_ERR_ARG;
  int rc = screen4_ready(s, "bcx_screen4_read");
  if (rc != BCX_OK) return rc;
  BCX_HIP(hipStreamSynchronize(s->stream));
  if (ld4_out) *ld4_out = s->ld4;
  if (count == 0) return BCX_OK;
  if (codes) BCX_HIP(hipMemcpy(codes, (const char*)s->A4 + (size_t)begin * s->ld4, (size_t)count * s->ld4, hipMemcpyDeviceToHost));
  std::vector<float> sb((size_t)count * 2);
  BCX_HIP(hipMemcpy(sb.data(), s->s4_sb + begin, (size_t)count * 8, hipMemcpyDeviceToHost));
  for (int64_t i = 0; i < count; ++i) {
    if (scales) scales[i] = sb[2 * i];
    if (bounds) bounds[i] = sb[2 * i + 1];
  }
  return BCX_OK;
}

// One launch of front4_kernel, and only that, against a caller's query and a caller's sentinel rows (no refine, no resolve, no
// tail, no counters): what it listed and what its second stage settled.  The query and DevState (active, qscale, qexp) are set
// as bcx_argmax_correlation sets them; afterwards DevState, the query and the sentinel rows are what they were.
extern "C" int bcx_screen4_probe(bcx_solver* s, const double* query_host, const int32_t* sentinels, int32_t* n_waves_out,
                                 int32_t* counts, int32_t* list, int32_t list_stride, void* partials) {
  if (!s || !query_host || !sentinels || !n_waves_out || list_stride < 0) return BCX_ERR_ARG;
  for (int i = 0; i < BCX_S4_SENTINELS; ++i)       // every index the kernel is handed is checked here
    if (!(sentinels[i] == -1 || (sentinels[i] >= 0 && (int64_t)sentinels[i] < s->cfg.n_local))) {
      s->err = "bcx_screen4_probe: sentinel " + std::to_string(i) + " is neither -1 nor a local row";
      return BCX_ERR_ARG;
    }
  if (s->enq_unpolled) { s->err = "bcx_screen4_probe: iterations are enqueued; call bcx_build_poll first"; return BCX_ERR_STATE; }
  int rc = screen4_ready(s, "bcx_screen4_probe");
  if (rc != BCX_OK) return rc;
  DevState h;
  if ((rc = read_state(s, &h))) return rc;
  BCX_HIP(hipStreamSynchronize(s->stream));
  int32_t sent_was[BCX_S4_SENTINELS];
  std::vector<char> q_was((size_t)s->ld * 4);
  BCX_HIP(hipMemcpy(sent_was, s->s4_sent, sizeof sent_was, hipMemcpyDeviceToHost));
  BCX_HIP(hipMemcpy(q_was.data(), s->qst, q_was.size(), hipMemcpyDeviceToHost));
  double qn = 0.0;
  int E = 0;
  if ((rc = upload_query(s, query_host, false, &qn, &E))) return rc;
  DevState forced = h;
  forced.active = 1; forced.exact_mode = 0; forced.qscale = qn; forced.qexp = E;
  BCX_HIP(hipMemcpy(s->st, &forced, sizeof forced, hipMemcpyHostToDevice));
  BCX_HIP(hipMemcpy(s->s4_sent, sentinels, sizeof sent_was, hipMemcpyHostToDevice));
  int nw = 0;
  rc = bcx_launch_front4_probe(s, &nw);
  hipError_t e = hipStreamSynchronize(s->stream);
  // (put everything back whatever the launch said)
  BCX_HIP(hipMemcpy(s->st, &h, sizeof h, hipMemcpyHostToDevice));
  BCX_HIP(hipMemcpy(s->s4_sent, sent_was, sizeof sent_was, hipMemcpyHostToDevice));
  BCX_HIP(hipMemcpy(s->qst, q_was.data(), q_was.size(), hipMemcpyHostToDevice));
  if (rc != BCX_OK) return rc;
  BCX_HIP(e);
  *n_waves_out = nw;
  std::vector<int32_t> cnt((size_t)nw);
  BCX_HIP(hipMemcpy(cnt.data(), s->s4_counts, (size_t)nw * 4, hipMemcpyDeviceToHost));
  if (counts) memcpy(counts, cnt.data(), (size_t)nw * 4);
  if (list && list_stride > 0) {
    std::vector<int32_t> all((size_t)nw * BCX_S4_SEG_CAP);
    BCX_HIP(hipMemcpy(all.data(), s->s4_list, all.size() * 4, hipMemcpyDeviceToHost));
    for (int b = 0; b < nw; ++b) {
      int m = cnt[b] < s->s4_seg_cap ? cnt[b] : s->s4_seg_cap;
      if (m > list_stride) m = list_stride;
      if (m > 0) memcpy(list + (size_t)b * list_stride, all.data() + (size_t)b * BCX_S4_SEG_CAP, (size_t)m * 4);
    }
  }
  if (partials) BCX_HIP(hipMemcpy(partials, s->scr_partials, (size_t)nw * BCX_PARTIAL_BYTES, hipMemcpyDeviceToHost));
  return BCX_OK;
}

// OMP step diagnostics since construction: out4 = {steps, columns that left the passive set, from-scratch re-solves,
// columns that entered beyond the selected one}
extern "C" int bcx_omp_stats(bcx_solver* s, int64_t* out4) {
  if (!s || !out4) return BCX_ERR_ARG;
  DevState h;
  int rc = read_state(s, &h);
  if (rc != BCX_OK) return rc;
  for (int i = 0; i < 4; ++i) out4[i] = h.n_omp[i];
  out4[2] += s->opt_fallbacks;          // optimize() calls that needed the refined solve count as re-solves too
  return BCX_OK;
}

extern "C" int bcx_profile_scan(bcx_solver* s, int32_t on) {
  if (!s) return BCX_ERR_ARG;
  s->profile = on != 0;
  s->prof_every = on > 1 ? on : 1;      // on = N > 1: time every N-th scan launch
  s->prof_tick = 0;
  s->prof_ms = 0.0;
  s->prof_launches = 0;
  s->prof_used = 0;
  return BCX_OK;
}

extern "C" int bcx_profile_read(bcx_solver* s, double* scan_ms_total, int64_t* scan_launches) {
  if (!s) return BCX_ERR_ARG;
  if (scan_ms_total) *scan_ms_total = s->prof_ms;
  if (scan_launches) *scan_launches = s->prof_launches;
  return BCX_OK;
}

// dev builds (-DBCX_TIMING): phase time stamps (100 MHz ticks) of the last merged tail; not in include/bcx.h
extern "C" int bcx_debug_stamps(bcx_solver* s, long long* out32) {
  DevState h;
  int rc = read_state(s, &h);
  if (rc != BCX_OK) return rc;
  for (int i = 0; i < 32; ++i) out32[i] = h.dbg_t[i];
  return BCX_OK;
}

// dev builds: raw copy of the weight back-up buffer (debug digests of nnls_grid.hip with -DBCX_DEBUG_GRID)
extern "C" int bcx_debug_wbak(bcx_solver* s, double* out, int32_t count) {
  if (!s || !s->nn_wbak || count > s->gram_cap) return BCX_ERR_ARG;
  BCX_HIP(hipDeviceSynchronize());
  BCX_HIP(hipMemcpy(out, s->nn_wbak, (size_t)count * sizeof(double), hipMemcpyDeviceToHost));
  return BCX_OK;
}
