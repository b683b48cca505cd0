// Internal definitions shared by the gfx950 kernels and the C-ABI host layer.
// Not part of the public boundary (that is include/bcx.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include <utility>
#include <vector>
#include "../../include/bcx.h"
#include "dev_buf.h"
#include "host_err.h"

#define BCX_CHUNK_ROWS 1024      // rows per column-sum chunk (fixed summation tree, shard-count independent)
#define BCX_MAX_CAND 64          // candidate rows re-scored in fp64 per shard per iteration
#define BCX_REC_HDR 4            // record header doubles: score, global index, norm, flags
#define BCX_REC_VALID 1.0
#define BCX_REC_OVERFLOW 2.0
#define BCX_MAX_D BCX_MAX_ROW_LENGTH   // include/bcx.h
#define BCX_SCAN_THREADS 256
#define BCX_APPLY_THREADS 256

enum { HALT_NONE = 0, HALT_DONE = 1, HALT_LIMIT = 2, HALT_NEED_EXACT = 3, HALT_EXCHANGE_TIMEOUT = 4, HALT_GRID_TIMEOUT = 5 };
enum { OMP_IDLE = 0, OMP_DONE = 1, OMP_FAST_TRY = 2, OMP_FAST_ACCEPT = 3, OMP_GENERAL = 4,
       OMP_OPT_FALLBACK = 5 };   // optimize_lh_kernel asks for the refined solve of nnls_grid.hip (its Newton check failed)

// Per-workgroup result of the correlation scan, stored as separate arrays (coalesced reads in the
// resolve step): the two best upper bounds with their local row indices, a bound on everything else
// the workgroup saw, and the best lower bound.  (For fp64 storage U == L == the score.)
struct PartialView {
  double *U1, *U2, *U3, *L;
  int32_t *i1, *i2;
};
#define BCX_PARTIAL_BYTES 40   // per workgroup: 4 doubles + 2 int32
#define BCX_MAX_PARTIALS 2048
// 8-bit screening tier (screen8.hip): survivors per iteration that the refine kernel re-scores from the stored rows, and the
// words of its device-side record
#define BCX_SCREEN_MAX_SURV 256
enum { SCR_ARMED = 0,       // the iteration in flight (or the one that halted) was screened by the tier
       SCR_ITERS = 1,       // iterations screened
       SCR_SURVIVORS = 2,   // rows re-scored from the stored rows, summed over the iterations that did not overflow
       SCR_OVERFLOWS = 3,   // iterations whose capture overflowed (a third survivor in one wave, or too many)
       SCR_REDOS = 4,       // halted tier iterations redone with the storage-precision scan
       SCR4_ITERS = 5,      // iterations that went through the 4-bit front pass (screen4.hip)
       SCR4_LISTED = 6,     // rows the front pass listed for the second stage, summed over those iterations
       SCR4_OVERFLOWS = 7,  // list segments that were full (words 5 to 8 are booked by refine_kernel, in the same iteration)
       SCR4_LAST = 8,       // 1 when the last iteration refine_kernel saw went through the 4-bit front pass: at a halt, that the
                            // halted iteration was a 4-bit one (the kernels of later iterations return at once)
       SCR_WORDS = 9 };
// 4-bit front tier: entries per wave in the list buffer (tools/screen4_model.py), sentinel rows
#define BCX_S4_SEG_CAP 1024
#define BCX_S4_SENTINELS 64
static inline __host__ __device__ PartialView partial_view(void* base, int n) {
  PartialView v;
  v.U1 = (double*)base; v.U2 = v.U1 + n; v.U3 = v.U2 + n; v.L = v.U3 + n;
  v.i1 = (int32_t*)(v.L + n); v.i2 = v.i1 + n;
  return v;
}

// Peer mailbox: the per-iteration record exchange of a row-sharded build without a host-side collective.
// Every shard owns one fine-grained device allocation, mapped by all peers (hipIpc):
//   flags [2][world] u64  -- sequence number of the record in slot [parity][source shard]
//   slots [2][world][d+4] doubles, starting at off_slots
// Exchange number `seq` uses parity seq & 1: a shard stores its record into slot [parity][rank] of every
// mailbox, fences, stores seq into the matching flags, then waits until its own flags [parity][*] reach
// seq.  A peer can be at most one exchange ahead (it needs this shard's next record to go further), so two
// parities suffice.  Sequence numbers never restart during the life of the solver.
struct Mailbox {
  void* const* peers;          // world mailbox base addresses (device array; [rank] is this shard's own)
  unsigned long long* seq;     // exchanges completed so far (device word; identical on every shard)
  int32_t* probe;              // result of bcx_exchange_probe: 1 ok, -1 timeout, -2 payload mismatch
  unsigned long long* stat;    // [5] ranks whose record did not arrive before the timeout (bit per rank & 63), [6] that exchange's number;
                               // [0] exchanges timed, [1] sum / [2] max of the wait for the peers' records, [3] sum / [4] max
                               // of the whole exchange (own stores + wait), wall_clock64 ticks (100 MHz); bcx_exchange_stats
  int world, rank, recw;
  unsigned off_slots;
  long long timeout_ticks;     // wall_clock64 ticks (100 MHz) before a wait gives up
};

static inline unsigned bcx_mailbox_slot_offset(int world) { return (unsigned)((2u * world * 8u + 255u) / 256u * 256u); }

// Replicated solver state (device resident; every shard holds an identical copy).
struct DevState {
  int64_t itrs;        // loop iterations requested by the current build() call
  int64_t it;          // loop iterations consumed so far in this call
  int32_t active;      // kernels of the current call do work only while this is 1
  int32_t halt;        // HALT_*
  int32_t retried;     // retried_already (snnls.py:40)
  int32_t limit;       // reached_numeric_limit
  int32_t k;           // slots in the sparse weight list
  int32_t since_refresh;
  int32_t exact_mode;  // current iteration's scan was exact (no candidate window)
  int32_t zero_row;    // first zero-norm local row + 1 (0 = none)
  int32_t no_monotone; // check_error_monotone=False (snnls.py:9,45,56): no error comparison, no revert, retry flag never cleared
  int32_t np;          // size of the passive set P (OMP / optimize)
  int32_t hvalid;      // hinv == inverse of gram[P,P] and P == {slots with weight > 0}
  int32_t hlo_valid;   // hinv_lo holds the low words of that inverse (omp_lh.hip keeps it in double-double); 0 after any
                       // kernel that rewrote hinv in plain doubles
  // multi-kernel OMP step (nnls.hip): decisions handed from kernel to kernel
  int32_t omp_mode;    // OMP_* below
  int32_t omp_slot, omp_fresh, omp_checked, omp_p;
  int32_t omp_ill;     // a Schur complement below 1e-4 of its diagonal was seen: the Gram system is
                       // ill-conditioned, every step takes the refined general solve from now on
  int64_t omp_f;
  double omp_nf, omp_gff, omp_cf, omp_t, omp_inv;
  double tol;          // bc.util.TOL at build() time
  double err;          // ||A w - b||
  double nw;           // ||A w|| (1 when zero, giga.py:23)
  double bnorm;        // ||b||
  double sigma;        // sum of row norms (frankwolfe.py:25)
  int64_t n_exact;     // diagnostics: iterations that needed the exact fp64 scan (candidate window overflow)
  int64_t n_cand;      // diagnostics: candidate rows re-scored in fp64, summed over iterations
  int64_t n_resolved;  // diagnostics: resolve passes
  int64_t n_omp[4];    // diagnostics (omp_lh.hip): OMP steps, columns that left, from-scratch re-solves, extra columns entered
  double qscale;       // norm of the query vector AS STORED for the scan (error bound of the fp32 scan scales with it)
  int32_t qexp;        // the fp32 query holds q * 2^-qexp (apply_common.h store_query); a low-precision score that leaves
  int32_t qexp_pad;    // the scan unre-scored is multiplied back by 2^qexp (resolve_core.h)
  long long dbg_t[32]; // phase time stamps of the last tail (dev builds with -DBCX_TIMING, tools/tail_timing.py)
};

struct bcx_solver {
  bcx_config cfg;
  hipStream_t stream = nullptr;
  std::string err;
  int ld = 0;               // row stride (elements) of the stored normalised matrix
  int elem = 4;             // bytes per stored element
  int qelem = 4;            // bytes per element of the storage-precision query
  int ld64 = 0;             // row stride (doubles) of A64 / q64 (d rounded up to even)
  DevBuf<char> An;          // n_local x ld, fp32 or fp64, rows normalised to unit norm
  DevBuf<double> A64;       // n_local x ld64 raw rows (optional)
  DevBuf<double> norms;     // n_local
  DevBuf<double> chunk_sums;     // n_chunks x (d+1)
  int64_t n_chunks = 0;
  DevBuf<char> staging;     // upload staging when raw rows are not kept
  DevBuf<DevState> st;
  DevBuf<double> b;         // d
  DevBuf<double> bn;        // d (GIGA)
  DevBuf<double> xw;        // d
  DevBuf<double> q64;       // 2 x ld64 query vectors (fp64, used by the exact re-score)
  DevBuf<char> qst;         // 2 x ld query vectors in storage precision (read by the scan)
  DevBuf<double> tmp;       // 4 x d scratch
  DevBuf<char> partials;        // PartialView storage
  int n_partials = 0;
  DevBuf<double> rec_local;      // (d+4) record produced by this shard when world_size == 1
  DevBuf<double> fin_part;       // finalize: sums of groups of chunk sums
  // peer mailbox (bcx_exchange_*): device-side record exchange for world_size > 1
  DevBuf<char> mbox;             // this shard's mailbox (fine-grained device memory, exported over hipIpc)
  std::vector<void*> peer_mbox;  // mapped mailboxes by rank ([rank] == mbox)
  DevBuf<void*> peer_tab;        // device copy of peer_mbox
  DevBuf<unsigned long long> xseq;      // [0] exchanges completed; [1..5] timing statistics, [6] late ranks (bit mask) and [7] the exchange
                                        // number of the last timeout (Mailbox::stat[0..6])
  DevBuf<int32_t> xprobe;
  DevBuf<double> rec_gather;     // world x (d+4): records of the last exchange (input of the OMP apply kernels)
  bool exchange_ready = false;
  double exchange_timeout_s = 20.0;
  // sparse weight list (selection order), grown on demand
  int64_t cap = 0;
  DevBuf<int64_t> act_idx;       // global row index per slot
  DevBuf<double> act_w;          // weight per slot
  DevBuf<double> act_rows;       // cap x d raw rows of the slots (replicated)
  DevBuf<double> act_norm;       // norm per slot
  // OMP / optimize(): Gram system over the slots
  DevBuf<double> gram;           // cap x cap
  DevBuf<double> hinv;           // cap x cap inverse of the passive block
  DevBuf<double> hinv_lo;        // its low words (double-double inverse of the OMP step, omp_lh.hip)
  DevBuf<double> cvec;           // cap : a_j . b
  DevBuf<int32_t> plist;         // passive list (slot ids)
  DevBuf<int32_t> ppos;          // slot -> position in plist or -1
  DevBuf<double> nn_x;           // cap
  DevBuf<double> nn_z;           // cap
  DevBuf<double> nn_wv;          // cap
  DevBuf<double> nn_tmp;         // 16*cap: position scratch t0..t3 = the first quarter of the exchange ring (grid_lh.h)
  DevBuf<int32_t> nn_flag;       // cap: bit0 in problem set S, bit1 rejected, bit2 remove
  DevBuf<double> nn_wbak;        // cap: weights before the step (revert on monotone failure)
  DevBuf<double> nn_xr;          // 2*cap: row-phase exchange of the OMP step (omp_lh.hip)
  int64_t gram_cap = 0;
  DevBuf<double> gram_work;      // optimize(): slice partials of the Gram kernel (moments.hip), grown on demand
  DevBuf<char> warm_buf;         // optimize(): buffers of the warm start (csrc/warm.hip), grown on demand
  int64_t opt_warm = 0, opt_warm_failed = 0;   // optimize() calls that started warm / whose warm start was rejected by the closing check
  int64_t k_ub = 0;              // host upper bound of the slot count (grid sizing of the multi-kernel OMP step)
  DevBuf<unsigned long long> grid_counter;      // [0] arrival counter of the grid barriers, [1] barrier base of the next OMP step
  uint64_t grid_epoch = 0;       // fused OMP launches since the counter was reset (bcx_build_begin)
  int64_t opt_fallbacks = 0;     // optimize() calls that took the refined solve after the incremental one's check failed (bcx_omp_stats)
  bool grid_dirty = false;       // optimize() advanced grid_counter[0] past the OMP step's base [1]: re-zero both before the next OMP step
  size_t omp_lds_allowed = 0;
  // trace of the current build() call
  int64_t trace_cap = 0;
  DevBuf<int64_t> tr_sel;
  DevBuf<double> tr_err;
  DevBuf<int32_t> tr_status;
  bool finalized = false;
  int64_t rows_loaded = 0;
  // 8-bit screening tier (screen8.hip)
  DevBuf<char> Aq;               // n_local x ld8 codes
  DevBuf<float2> scr_sb;         // n_local x (fp32 scale, fp32 bound)
  DevBuf<char> scr_partials;     // per-wave partials of the screen kernel
  DevBuf<unsigned long long> scr_stat;      // SCR_* words
  int ld8 = 0;
  bool scr_enabled = true;       // off: BCX_SCREEN8=0 (dev switch)
  int scr_dropped = 0;           // 1: dropped by the overflow rule until bcx_reset, 2: no memory for the shadow
  bool scr_valid = false;        // the shadow matches the stored rows
  bool scr_batch = false;        // the iterations enqueued last went through the tier
  float scr_build_ms = 0.f;
  uint64_t scr_ovf_at[4] = {0, 0, 0, 0};   // SCR_ITERS stamps of the last four halts (drop rule, api.hip)
  int64_t scr_halts = 0;
  int scr_n_in = 0;              // partials in scr_partials after the last tier iteration that was enqueued
  // 4-bit front tier (screen4.hip): in front of the 8-bit tier for the single-query algorithms on one shard
  DevBuf<char> A4;               // n_local x ld4 bytes of 4-bit codes
  DevBuf<float2> s4_sb;          // n_local x (fp32 scale4, fp32 bound4)
  DevBuf<int32_t> s4_list;       // BCX_MAX_PARTIALS segments of BCX_S4_SEG_CAP row indices
  DevBuf<int32_t> s4_counts;     // BCX_MAX_PARTIALS entries: rows a wave wanted to list
  DevBuf<int32_t> s4_sent;       // BCX_S4_SENTINELS row indices (-1: none) the last refine_kernel left for the next front pass
  int ld4 = 0;
  int s4_seg_cap = BCX_S4_SEG_CAP;   // entries of a segment in use; dev switch BCX_SCREEN4_SEGCAP=<n> lowers it (tests of the overflow path)
  bool s4_enabled = true;        // off: BCX_SCREEN4=0 (dev switch)
  int s4_dropped = 0;            // 1: dropped to the 8-bit tier by the redo rule until bcx_reset, 2: no memory for the second shadow
  bool s4_valid = false;         // the 4-bit shadow matches the stored rows
  int s4_warm = 2;               // plain 8-bit iterations still to run before the last refine has left usable sentinel rows
  uint64_t s4_ovf_at[4] = {0, 0, 0, 0};   // SCR4_ITERS stamps of the last four halted 4-bit iterations (drop rule, api.hip)
  int64_t s4_halts = 0;         // since bcx_reset
  int64_t s4_redos = 0, s4_drops = 0;   // since construction (bcx_screen4_stats)
  bool enq_unpolled = false;     // iterations were enqueued and bcx_build_poll has not been called since (bcx_screen4_probe refuses)
  // measurement
  bool profile = false;
  bool prof_now = false;
  int prof_every = 1;
  int64_t prof_tick = 0;
  double prof_ms = 0.0;
  int64_t prof_launches = 0;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> prof_events;
  size_t prof_used = 0;

  // The peers' mailboxes are unmapped here, before the members go: this shard's own mailbox (one of them) is freed after.
  void close_peers() {
    for (void* p : peer_mbox)
      if (p && p != mbox.get()) (void)hipIpcCloseMemHandle(p);
    peer_mbox.clear();
  }
  ~bcx_solver() {
    close_peers();
    for (auto& ev : prof_events) { (void)hipEventDestroy(ev.first); (void)hipEventDestroy(ev.second); }
  }
};

// ---- kernel launchers (defined in the .hip files) ------------------------
int bcx_launch_ingest(bcx_solver* s, const void* src, int src_dtype, int64_t ld_src, int64_t row_begin, int64_t rows,
                      int center);
int bcx_launch_finalize(bcx_solver* s, int have_b, const double* gathered, int64_t n_gathered);
int bcx_launch_scan(bcx_solver* s, int exact);
int bcx_launch_resolve(bcx_solver* s, double* send_dev, int exact);
int bcx_launch_begin(bcx_solver* s, int64_t itrs, double tol);
int bcx_launch_apply(bcx_solver* s, const double* recv_dev);
int bcx_launch_tail(bcx_solver* s, int exact);
int bcx_launch_omp_fused(bcx_solver* s, int exact);   // nnls.hip: scan partials -> OMP step in one launch; 1 = not applicable
int bcx_launch_tail_exchange(bcx_solver* s, int exact);   // resolve + mailbox exchange + apply (world_size > 1)
int bcx_launch_exchange_probe(bcx_solver* s);
Mailbox bcx_mailbox(const bcx_solver* s);
int bcx_launch_resume_exact(bcx_solver* s);
int bcx_launch_error_refresh(bcx_solver* s);
int bcx_launch_optimize(bcx_solver* s, double tol);
// moments.hip: G = rows rows^T (k x k, both triangles) on the fp64 matrix cores; work: bcx_gram_rows_scratch_bytes(k, d) bytes
int64_t bcx_gram_rows_scratch_bytes(int k, int d);
int bcx_gram_rows(hipStream_t st, const double* rows, int k, int d, int64_t ld, double* G, int64_t ldg, double* work);
// the same by the tiled kernel alone (no hand-off between workgroups inside a launch); work: bcx_gram_tiled_scratch_bytes(k, d) bytes
int64_t bcx_gram_tiled_scratch_bytes(int k, int d);
int bcx_gram_rows_tiled(hipStream_t st, const double* rows, int k, int d, int64_t ld, double* G, int64_t ldg, double* work);
// gram.hip: the call counter of the stream-K kernel and the check of its time-out word (first 8 bytes of the scratch)
unsigned long long bcx_gram_sk_epoch_now();
int bcx_gram_sk_timed_out(hipStream_t st, const double* work, unsigned long long since);
int bcx_scan_grid(const bcx_solver* s);
// api.hip: the words behind bcx_solver::grid_counter, allocated zero-filled on first use; the callers reset what they use per call
#define BCX_GRID_WORDS 32   // [0] arrivals, [1] barrier base of the next OMP step, [16] (its own 128-byte line) the barrier index
                            // word of the split form (GridSync::gen)
int bcx_ensure_grid_counter(bcx_solver* s);
// screen8.hip
bool bcx_screen_on(const bcx_solver* s);
int bcx_screen_build(bcx_solver* s);
int bcx_launch_screen(bcx_solver* s);
int bcx_launch_resume_store(bcx_solver* s);
int bcx_launch_refine(bcx_solver* s, int n_in, bool four);   // four: the partials come from the 4-bit front pass
// screen4.hip
bool bcx_screen4_on(const bcx_solver* s);
int bcx_screen4_build(bcx_solver* s);
int bcx_launch_screen4(bcx_solver* s);
int bcx_launch_front4_probe(bcx_solver* s, int* n_waves);   // front4_kernel alone, the plan of bcx_launch_screen4 (bcx_screen4_probe)
// proj.hip: the likelihood tables of proj_math.h (PJT_DOUBLES doubles) in the current device's memory; nullptr: no memory
const double* proj_tables();

#ifdef BCX_TIMING
#define BCX_STAMP(st, i) do { if (threadIdx.x == 0) (st)->dbg_t[i] = wall_clock64(); } while (0)
#else
#define BCX_STAMP(st, i) do {} while (0)
#endif

#define BCX_HIP(call)                                                        \
  do {                                                                       \
    hipError_t _e = (call);                                                  \
    if (_e != hipSuccess) {                                                  \
      s->err = std::string(#call) + ": " + hipGetErrorString(_e);            \
      return BCX_ERR_HIP;                                                    \
    }                                                                        \
  } while (0)
