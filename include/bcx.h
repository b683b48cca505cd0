/*
 * bcx.h -- C ABI of the MI355X (gfx950) coreset-construction engine.
 *
 * One shared library (libbcx.so, built by hipcc --offload-arch=gfx950) replaces
 * the NumPy/SciPy arithmetic behind the reference's sparse-NNLS solvers.  The
 * reference (trevorcampbell/bayesian-coresets @ v0.9.1) has no FFI of its own
 * (it is pure Python), so each entry point below names the reference interface
 * whose work it takes over; INTEGRATION.md shows the ctypes stub a maintainer
 * of the reference would add.
 *
 * Conventions: plain C types only; every function returns an int status
 * (BCX_OK == 0, negative == error, message via bcx_last_error); no C++
 * exception crosses the boundary; the opaque handle owns all device memory;
 * outputs are caller-allocated HOST buffers unless a parameter says "dev";
 * device pointers are passed as const void* (from torch.Tensor.data_ptr()).
 * One host thread per handle.
 *
 * The Python binding (bayesiancoresets_amd/_abi.py) PARSES THIS FILE at import -- signatures, constants and the two structs are
 * written down here only -- and refuses to load a declaration outside this grammar: one prototype per `;` with every parameter
 * named; parameters int32_t, int64_t, uint64_t, double or a pointer (any pointer is passed as an address), `(void)` for none;
 * returns int, int32_t, int64_t or const char*; struct fields of the same types; anonymous enums with an explicit value for
 * every name; `#define BCX_NAME <integer>`.  No arrays, function pointers or structs by value.
 */
#ifndef BCX_H
#define BCX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct bcx_solver bcx_solver;

/* ---- enums ---------------------------------------------------------- */
enum { BCX_ALG_GIGA = 0, BCX_ALG_FW = 1, BCX_ALG_OMP = 2 };
enum { BCX_F32 = 0, BCX_F64 = 1, BCX_F16 = 2 };   /* BCX_F16: storage of the normalised rows only */

/* return codes */
enum {
  BCX_OK = 0,
  BCX_ERR_ARG = -1,        /* bad argument / call order */
  BCX_ERR_HIP = -2,        /* HIP runtime failure (message has hipGetErrorString) */
  BCX_ERR_ZERO_ROW = -3,   /* a data row has zero norm: reference raises ValueError (giga.py:11-12) */
  BCX_ERR_ZERO_B = -4,     /* ||b|| == 0 for GIGA: reference raises NumericalPrecisionError (giga.py:16-17) */
  BCX_ERR_NOMEM = -5,
  BCX_ERR_STATE = -6,      /* solver not initialised / already latched where not allowed */
  BCX_ERR_EXCHANGE = -7,   /* peer mailbox: a shard's record did not arrive in time (see bcx_exchange_attach) */
  BCX_ERR_TIMEOUT = -8     /* a wait between workgroups of one launch expired (GPU shared / preempted): the result is not valid */
};

/* per-iteration status written to the trace (snnls.py:41-74 outcome of one loop iteration) */
enum {
  BCX_IT_OK = 0,            /* step accepted */
  BCX_IT_FAIL_SELECT = 1,   /* NumericalPrecisionError raised inside _select   (giga.py:28-29) */
  BCX_IT_FAIL_REWEIGHT = 2, /* NumericalPrecisionError raised inside _reweight (giga.py:50-51, frankwolfe.py:33-34) */
  BCX_IT_FAIL_MONOTONE = 3  /* error increased, weights reverted               (snnls.py:58-61) */
};

typedef struct bcx_config {
  int32_t alg;             /* BCX_ALG_*                                                          */
  int32_t store_dtype;     /* BCX_F32: normalised rows stored fp32 (default); BCX_F64: exact mode;
                              BCX_F16: fp16 rows (half the bytes per iteration; needs keep_exact_rows for the fp64 re-score) */
  int32_t keep_exact_rows; /* 1: also keep the raw fp64 rows resident (exact reweight + fp64 rescue) */
  int32_t device;          /* HIP device ordinal                                                  */
  int32_t d;               /* projection dimension (columns of the N x d vector matrix)           */
  int32_t world_size;      /* number of row shards (1 = single GPU)                               */
  int32_t rank;            /* this shard                                                          */
  int32_t refresh_every;   /* recompute xw = sum_j w_j A[:,j] from the active rows every this many accepted steps (0 = default 64) */
  int64_t n_local;         /* rows held by this shard                                             */
  int64_t n_global;        /* rows over all shards                                                */
  int64_t row_offset;      /* global index of local row 0 (contiguous row blocks, lowest index wins ties) */
} bcx_config;

/* ---- lifetime -------------------------------------------------------- */
/* Replaces SparseNNLS.__init__ storage (snnls/snnls.py:9-16): allocates An (N x d, store_dtype),
 * norms (fp64), optional raw rows (fp64) and the replicated O(d) solver state. */
/* Longest supported row (the projection dimension d of the vectors; the reference takes any): a bound on the argument, not
 * a capacity of any kernel.  Up to 4096 floats / 2048 doubles of stored row the scan keeps the query in registers; longer rows
 * take a one-wave-per-row form with the query in LDS (its tail beyond 144 KiB is read from global memory), the O(d) state
 * kernels keep their five d-vectors in LDS up to d = 3584 and in global scratch beyond, the constructor pass adds column sums
 * in LDS up to d = 18432 and in place beyond, the OMP step takes its multi-kernel form once three d-vectors exceed its LDS
 * budget, and row shards of more than 18432 values exchange their records by all-gather instead of the peer mailbox. */
#define BCX_MAX_ROW_LENGTH 1048576
int bcx_create(const bcx_config* cfg, bcx_solver** out);
int bcx_destroy(bcx_solver* s);
/* Last error text for this handle (or for a failed bcx_create when s == NULL). */
const char* bcx_last_error(const bcx_solver* s);
/* Use the caller's HIP stream (torch.cuda.current_stream().cuda_stream); NULL = default stream. */
int bcx_set_stream(bcx_solver* s, void* hip_stream);

/* ---- ingest: GIGA/FW/OMP constructors (giga.py:8-13, frankwolfe.py:7-13, orthopursuit.py:9-15) --- */
/* Copy `rows` rows starting at local row `row_begin` from src (host or device memory, fp32 or fp64,
 * row-major with leading dimension ld elements), compute their norms (fp64), store the normalised
 * rows and accumulate per-chunk column sums / norm sums.  May be called repeatedly (row shards,
 * streaming upload).  A zero-norm row is reported by bcx_finalize (BCX_ERR_ZERO_ROW). */
int bcx_load_rows(bcx_solver* s, const void* src, int32_t src_is_device, int32_t src_dtype,
                  int64_t row_begin, int64_t rows, int64_t ld);
/* The same with options.  BCX_LOAD_CENTER_ROWS: subtract every row's mean before anything else, i.e. the rows are
 * raw log-likelihoods and the constructor pass applies the projector's centring (projector.py:21) itself -- the row
 * is in registers between the norm and the stores, so a projection that feeds HilbertCoreset is written once and read
 * once instead of taking a separate centring pass.  The caller's buffer is left as it is (uncentred). */
#define BCX_LOAD_CENTER_ROWS 1
int bcx_load_rows_flags(bcx_solver* s, const void* src, int32_t src_is_device, int32_t src_dtype,
                        int64_t row_begin, int64_t rows, int64_t ld, int32_t flags);
/* Number of row chunks on this shard and rows per chunk; chunk sums are (d+1) doubles each:
 * d column sums followed by the sum of row norms.  Device pointer for the all-gather across shards. */
int bcx_chunk_sums(bcx_solver* s, const void** dev_ptr, int64_t* n_chunks, int64_t* chunk_rows);
/* Copy this shard's chunk sums into a caller-owned device buffer (e.g. a torch tensor that is then
 * all-gathered); asynchronous on the stream.  cap_chunks >= n_chunks. */
int bcx_export_chunk_sums(bcx_solver* s, void* dst_dev, int64_t cap_chunks);
/* Finish construction.  b_host (d doubles) overrides the column sums when non-NULL -- the reference
 * solver constructors take b from the caller (snnls.py:9; hilbert.py:24 passes vecs.sum(axis=0)).
 * gathered_sums_dev (optional): chunk sums of ALL shards in global chunk order (n_gathered chunks),
 * summed in that fixed order so b and sum(Anorms) are bit-identical for any shard count.
 * Returns BCX_ERR_ZERO_ROW / BCX_ERR_ZERO_B exactly where the reference constructors raise. */
int bcx_finalize(bcx_solver* s, const double* b_host, const void* gathered_sums_dev, int64_t n_gathered);

/* ---- the hot loop: SparseNNLS.build (snnls.py:31-79) ---------------------------------------- */
/* Begin a build() call of `itrs` loop iterations (resets the per-call retry flag, snnls.py:40;
 * tol is bc.util.TOL read at call time, giga.py:28).  Returns 1 in *skip if the reference would
 * return immediately (latched numeric limit snnls.py:32-34, or no data :36-38). */
int bcx_build_begin(bcx_solver* s, int64_t itrs, double tol, int32_t* skip);
/* Enqueue one greedy iteration up to the shard exchange: correlation scan over the local rows
 * (giga.py:31-38 / frankwolfe.py:16-17 / orthopursuit.py:18-26) + exact fp64 re-score of the
 * candidates; writes this shard's record {score, global index, norm, flags, row[d]} (d+4 doubles)
 * to send_dev.  Asynchronous on the stream. */
int bcx_step_scan(bcx_solver* s, void* send_dev);
/* Enqueue the replicated part: pick the winner among world_size records at recv_dev (max score,
 * lowest global index), OMP negative direction (orthopursuit.py:27-35), reweight
 * (giga.py:40-64 / frankwolfe.py:19-40 / orthopursuit.py:37-42), monotone check / revert / retry /
 * latch (snnls.py:56-74), and the next query vector.  Asynchronous on the stream. */
int bcx_step_apply(bcx_solver* s, const void* recv_dev);
/* Enqueue up to `itrs` whole iterations (scan + resolve + apply) without host round trips: single
 * shard, or row shards after bcx_exchange_attach (the record exchange then happens on the device).
 * bcx_build_enqueue_exact enqueues one iteration with the exact fp64 scan (after *need_exact). */
int bcx_build_enqueue(bcx_solver* s, int64_t itrs);
int bcx_build_enqueue_exact(bcx_solver* s);
/* ---- peer mailbox: device-side record exchange between row shards ------------
 * Replaces the per-iteration all-gather of bcx_step_scan / bcx_step_apply by direct stores into the
 * peers' mailboxes over xGMI, issued by the iteration's own tail kernel, so a sharded build needs no
 * host-side collective and no host round trip per iteration.  One process per GPU on one node:
 *   bcx_exchange_export  allocate this shard's mailbox and return its hipIpc handle (64 bytes);
 *   (the caller all-gathers the handles, e.g. torch.distributed.all_gather_object)
 *   bcx_exchange_attach  map the mailboxes of all shards (handles in rank order, handle_bytes apart);
 *                        timeout_s bounds every wait for a peer (<= 0: default 20 s), after which the
 *                        build stops and bcx_build_poll returns BCX_ERR_EXCHANGE instead of hanging;
 *   bcx_exchange_probe   COLLECTIVE: one exchange with a known payload; *result = 1 if every shard's
 *                        record arrived intact, -1 timeout, -2 payload mismatch;
 *   bcx_exchange_set_timeout  change the bound on every later wait;
 *   bcx_exchange_disable go back to the host-driven exchange (e.g. after a failed probe).
 *   bcx_exchange_stats   device-side time stamps of the exchanges since the last reset: how many, mean / max microseconds
 *                        this shard waited for the slowest peer's record after posting its own, mean / max of the whole
 *                        exchange step (own stores + wait); any output may be NULL; reset != 0 clears the counters.
 * All shards must issue the same sequence of exchanges (they do: the solver state is replicated). */
int bcx_exchange_export(bcx_solver* s, void* handle_out, int32_t handle_bytes);
int bcx_exchange_attach(bcx_solver* s, const void* handles, int32_t handle_bytes, double timeout_s);
int bcx_exchange_probe(bcx_solver* s, int32_t* result);
int bcx_exchange_set_timeout(bcx_solver* s, double timeout_s);
int bcx_exchange_disable(bcx_solver* s);
int bcx_exchange_stats(bcx_solver* s, int64_t* n, double* wait_us_mean, double* wait_us_max, double* total_us_mean,
                       double* total_us_max, int32_t reset);
/* Synchronise and report.  *n_done = loop iterations consumed so far in this build() call;
 * *need_exact = 1 if the engine stopped before an iteration because the fp32 candidate window
 * overflowed (tie-heavy data) -- call bcx_step_scan_exact for that iteration and continue;
 * *limit = reached_numeric_limit (snnls.py:67). */
int bcx_build_poll(bcx_solver* s, int64_t* n_done, int32_t* need_exact, int32_t* limit);
/* Exact (all-fp64) variant of bcx_step_scan used for the overflow fallback and by store_dtype F64. */
int bcx_step_scan_exact(bcx_solver* s, void* send_dev);
/* Copy the trace of this build() call: per loop iteration the selected global index (-1 if select
 * failed), the error after the iteration and a BCX_IT_* status.  Arrays sized >= n_done. */
int bcx_build_trace(bcx_solver* s, int64_t* sel, double* err, int32_t* status, int64_t cap, int64_t* n_out);

/* ---- read-out: weights()/size()/error() (snnls.py:22-29), optimize() (:82-97), reset() (:18-20) -- */
int bcx_active_count(bcx_solver* s, int64_t* k);                 /* entries in the sparse weight list (any weight) */
int bcx_get_weights(bcx_solver* s, int64_t* idx, double* w, int64_t cap, int64_t* k); /* selection order */
int bcx_error(bcx_solver* s, double* err);
int bcx_optimize(bcx_solver* s, double tol, int32_t* accepted);
int bcx_reset(bcx_solver* s);
/* SparseNNLS(A, b, check_error_monotone) (snnls.py:9,16): on = 0 switches the per-iteration error comparison and the
 * revert off (snnls.py:45-47,56-62); the retry flag is then never refreshed, exactly as in the reference where the
 * refresh sits inside the monotone branch.  Default on.  Survives bcx_reset; call between build() calls only. */
int bcx_set_check_monotone(bcx_solver* s, int32_t on);
int bcx_reached_numeric_limit(bcx_solver* s, int32_t* limit);

/* ---- introspection / measurement ------------------------------------------------------------ */
/* Copy replicated vectors to the host for tests: which = 0:b 1:xw 2:query0 3:query1 (d doubles). */
int bcx_get_vector(bcx_solver* s, int32_t which, double* out);
/* Copy row norms of local rows [begin, begin+count) (Anorms, frankwolfe.py:10). */
int bcx_get_norms(bcx_solver* s, int64_t begin, int64_t count, double* out);
/* The stored (normalised) rows [begin, begin + count) as the scan reads them: count x ld elements of the storage type
 * (fp32, fp16 or fp64; ld = d rounded up to a multiple of 16 bytes, returned in *ld_out; elements beyond d are padding). */
int bcx_get_stored_rows(bcx_solver* s, int64_t begin, int64_t count, void* out, int32_t* ld_out);
/* One N-way correlation scan with a caller-supplied query (d doubles, host): *idx = arg-max_n of
 * An[n] . query (first maximum, global row index), *score = its exact fp64 value.  The select step of
 * SparseVI on projected vectors (sparsevi.py:49-56).  FW / OMP handles only. */
int bcx_argmax_correlation(bcx_solver* s, const double* query_host, int64_t* idx, double* score);
/* Time `reps` launches of the correlation-scan kernel alone with hipEvents on the solver's stream;
 * returns the mean milliseconds per launch and the algorithmic bytes one launch reads. */
int bcx_time_scan(bcx_solver* s, int32_t reps, int32_t exact, double* ms_per_launch, double* bytes_per_launch);
/* Diagnostics since construction: iterations that fell back to the exact fp64 scan, candidate rows re-scored
 * in fp64 (total) and resolve passes (candidates / resolves = mean candidates per iteration). */
int bcx_stats(bcx_solver* s, int64_t* exact_fallbacks, int64_t* candidates, int64_t* resolves);
/* The 8-bit screening tier (default path of bcx_build_enqueue for fp32 / fp16 storage, d <= 4096): every greedy iteration
 * streams a one-byte-per-element shadow of the stored rows, whose per-row error bound makes the scan a rigorous enclosure;
 * the few rows it cannot exclude are re-scored from the stored rows, then in fp64 as before, so selections do not change.
 * out8 = {1 if the next enqueued iteration goes through the tier, iterations screened, survivors re-scored from the stored
 * rows, capture overflows, iterations redone with the storage-precision scan (these are NOT exact fallbacks), drop state
 * (0 in use, 1 dropped until bcx_reset after 4 redone iterations within 256 screened ones, 2 no device memory for the
 * shadow, 3 switched off or not applicable), device bytes held by the tier, microseconds the last shadow build took}.
 * bcx_stats keeps its meaning: `candidates` counts rows re-scored in fp64.  With the 4-bit front pass (below) the redone
 * iterations count every tier iteration redone with the storage-precision scan, 8-bit and 4-bit alike; bcx_screen4_stats
 * gives the 4-bit ones on their own. */
int bcx_screen_stats(bcx_solver* s, int64_t* out8);
/* The 4-bit front pass in front of that tier (FW / OMP on one shard, wherever the 8-bit tier runs): an iteration streams a
 * half-byte-per-element second shadow against a threshold taken, in 8 bits, from the rows that led the previous iteration,
 * and reads the 8-bit shadow only for the rows it lists; selections do not change.
 * out8 = {1 if the iterations enqueued next go through it (after the one or two plain 8-bit iterations that give it its
 * first threshold), 4-bit iterations, rows listed, list segments that were full, halted 4-bit iterations that were redone,
 * state (0 in use, 1 dropped to the 8-bit tier until bcx_reset after 4 redone iterations within 256 4-bit ones, 2 no device
 * memory for the second shadow, 3 switched off or not applicable), device bytes of the second shadow, times it dropped}. */
int bcx_screen4_stats(bcx_solver* s, int64_t* out8);
/* Read back rows [begin, begin + count) of the shadow: codes (count x ld8 bytes, ld8 = d rounded up to 16, returned in
 * *ld8_out; value = (code - 128) * scale), per-row scales and per-row upper bounds of ||stored row - dequantised row||_2.
 * Builds the shadow if it is due (it is built before the first enqueued iteration after bcx_finalize). */
int bcx_screen_read(bcx_solver* s, int64_t begin, int64_t count, void* codes, float* scales, float* bounds, int32_t* ld8_out);
/* Diagnostics of the 4-bit front pass (tests hold the kernel to exact arithmetic with them; no solver path calls them).
 * Both build the two shadows if they are due and return BCX_ERR_STATE where the front pass does not apply (GIGA, fp64
 * storage, row shards, switched off, no device memory for the second shadow).
 * The read is the twin of the one above for the second shadow: codes (count x ld4 bytes, ld4 = ceil(d / 32) * 16, returned
 * in *ld4_out; element 8 w + k of a row in bits 4k..4k+3 of its dword w as code + 8, code in [-7, 7], padding nibbles 8;
 * value = code * scale4), per-row scale4 and per-row upper bounds bound4 of ||stored row - dequantised row||_2. */
int bcx_screen4_read(bcx_solver* s, int64_t begin, int64_t count, void* codes, float* scales, float* bounds, int32_t* ld4_out);
/* The probe runs ONE launch of the front pass kernel, and only that, with the launch plan of an iteration, against the
 * caller's query (d doubles, scaled and stored as by the argmax entry above) and the caller's 64 sentinel rows (each -1 = none
 * or a local row index; anything else: BCX_ERR_ARG, nothing is launched).  After synchronising it returns the number of waves
 * (= list segments = partials, at most BCX_SCREEN4_MAX_WAVES) in *n_waves_out, the rows every wave wanted to list in
 * counts[w], the first min(counts[w], segment capacity, list_stride) listed rows of wave w at list + w * list_stride, and in
 * `partials` what the second stage settled, as n_waves doubles each of U1, U2, U3, L followed by n_waves int32 each of i1, i2
 * (40 bytes per wave).  counts, list and partials may be NULL; otherwise they hold BCX_SCREEN4_MAX_WAVES waves.  The solver's
 * state, its query and its sentinel rows are restored: a build after a probe gives what it gives without one.
 * BCX_ERR_STATE when iterations are enqueued and bcx_build_poll has not been called since. */
#define BCX_SCREEN4_MAX_WAVES 2048
int bcx_screen4_probe(bcx_solver* s, const double* query_host, const int32_t* sentinels, int32_t* n_waves_out,
                      int32_t* counts, int32_t* list, int32_t list_stride, void* partials);
/* Sum of scan-kernel time recorded by hipEvents during bcx_build_enqueue: on = 1 times every scan launch,
 * on = N > 1 every N-th one (an event pair costs several microseconds of stream time), on = 0 stops. */
/* OMP step diagnostics since construction: out4 = {steps taken, columns that left the passive set, from-scratch re-solves
 * (the incremental inverse had drifted, or a reverted step; also optimize() calls whose incremental solve failed its closing
 * Newton check and were redone by the refined solve), columns that entered beyond the selected one}. */
int bcx_omp_stats(bcx_solver* s, int64_t* out4);
int bcx_profile_scan(bcx_solver* s, int32_t on);
int bcx_profile_read(bcx_solver* s, double* scan_ms_total, int64_t* scan_launches);
/* ---- device-native projection (projector.py:19-21 with the example likelihoods) --------------------
 * vecs[n][s] = loglik(z_n, theta_s) - mean over s, for family 0 = logistic (model_lr.py:25-32),
 * 1 = Poisson/softplus (model_poiss.py:25-38), 2 = Gaussian linear regression (model_linreg.py:4-10;
 * param = sigma^2).  Z_dev: N x ldz doubles (features in columns [0, D), response in column ycol for
 * families 1 and 2), theta_dev: S x ldt doubles.  Stateless; asynchronous on `stream`.
 *   write  : vecs (N x S) into out_dev; rowsum_dev: unused (may be NULL; earlier builds wanted N doubles of scratch)
 *   colsum : sum_n vecs[n][s] without materialising vecs (sparsevi.py:70-74); work_dev = 2048*S doubles
 *   select : arg-max_n vecs[n].resid / ||vecs[n]|| / S (sparsevi.py:49-51) -> result_dev = {double, int64};
 *            work_dev = 2048 doubles + 2048 int64 */
int bcx_project_write(void* stream, int32_t family, const void* Z_dev, int64_t N, int64_t ldz, int32_t D,
                      int32_t ycol, const void* theta_dev, int32_t S, int32_t ldt, double param,
                      void* out_dev, int64_t ldo, void* rowsum_dev);
 /* write_raw: the log-likelihoods WITHOUT the centring (one pass less); the rows are centred by whoever reads them, e.g.
  * bcx_load_rows_flags(..., BCX_LOAD_CENTER_ROWS) -- HilbertCoreset behind a device projector. */
int bcx_project_write_raw(void* stream, int32_t family, const void* Z_dev, int64_t N, int64_t ldz, int32_t D,
                          int32_t ycol, const void* theta_dev, int32_t S, int32_t ldt, double param,
                          void* out_dev, int64_t ldo);
/* The same for the POINTS of a coreset (sparsevi.py:38-39): rows that every shard holds and projects alike, so the kernel may
 * be chosen by their number (up to 4096 rows: 32 x 32 blocks straight from L2; the data rows of bcx_project_write keep one
 * kernel whatever their shard's size, so that row-sharded builds reproduce the single-shard one bit for bit).  center != 0:
 * centred rows as bcx_project_write, 0: raw as bcx_project_write_raw. */
int bcx_project_write_points(void* stream, int32_t family, const void* Z_dev, int64_t N, int64_t ldz, int32_t D,
                             int32_t ycol, const void* theta_dev, int32_t S, int32_t ldt, double param,
                             void* out_dev, int64_t ldo, int32_t center);
int bcx_project_colsum(void* stream, int32_t family, const void* Z_dev, int64_t N, int64_t ldz, int32_t D,
                       int32_t ycol, const void* theta_dev, int32_t S, int32_t ldt, double param,
                       void* colsum_dev, void* work_dev);
int bcx_project_select(void* stream, int32_t family, const void* Z_dev, int64_t N, int64_t ldz, int32_t D,
                       int32_t ycol, const void* theta_dev, int32_t S, int32_t ldt, double param,
                       const void* resid_dev, double resid_sum, void* result_dev, void* work_dev);
/* The select step with ALL of its scratch supplied by the caller (it then never touches the stream-ordered allocator):
 * work_dev holds bcx_project_select_scratch_bytes(family, N, S) bytes = 2048 doubles + 2048 int64 for the arg-max
 * reduction, then 32 bytes per row and 64-column group for the partial row moments. */
int64_t bcx_project_select_scratch_bytes(int32_t family, int64_t N, int32_t S);
int bcx_project_select_ws(void* stream, int32_t family, const void* Z_dev, int64_t N, int64_t ldz, int32_t D,
                          int32_t ycol, const void* theta_dev, int32_t S, int32_t ldt, double param,
                          const void* resid_dev, double resid_sum, void* result_dev, void* work_dev, int64_t work_bytes);
/* The two fused consumers on INDEXED rows of a standing matrix: row i of the virtual n_rows-row matrix is Z[rows[i]], rows_dev =
 * n_rows int64 indices in device memory, duplicates and any order allowed (a `randint` draw).  Every index must lie in [0, N):
 * the kernel does not check -- the caller validates the table before it uploads it.  Same kernel, launch plan and order of
 * every sum as the contiguous entries take for N = n_rows: the results are those of bcx_project_colsum / bcx_project_select_ws on
 * a contiguous copy of the indexed rows (same leading dimension and 16-byte alignment class), bit for bit; the select's
 * result_dev names the POSITION i in rows (first maximum).  n_rows = 0: zeros / (-inf, -1).  The row requests carry 32-bit
 * offsets from Z_dev (16-byte units for 16-byte aligned rows, elements otherwise): a matrix of more than 64 GiB / 32 GiB is
 * refused with BCX_ERR_ARG -- gather with bcx_gather_rows and call the contiguous entry instead.
 * Scratch as the contiguous entries: work_dev = 2048*S doubles (colsum), bcx_project_select_rows_scratch_bytes (select). */
int bcx_project_colsum_rows(void* stream, int32_t family, const void* Z_dev, int64_t N, int64_t ldz, int32_t D,
                            int32_t ycol, const void* theta_dev, int32_t S, int32_t ldt, double param,
                            const void* rows_dev, int64_t n_rows, void* colsum_dev, void* work_dev);
int64_t bcx_project_select_rows_scratch_bytes(int32_t family, int64_t n_rows, int32_t S);
int bcx_project_select_rows_ws(void* stream, int32_t family, const void* Z_dev, int64_t N, int64_t ldz, int32_t D,
                               int32_t ycol, const void* theta_dev, int32_t S, int32_t ldt, double param,
                               const void* rows_dev, int64_t n_rows, const void* resid_dev, double resid_sum,
                               void* result_dev, void* work_dev, int64_t work_bytes);
/* out_dev[i][0 .. C) = Z_dev[rows[i]][0 .. C) for i < n_rows (out_dev: n_rows x ldo doubles, caller-owned): a plain copy of the
 * indexed rows, 16-byte pieces where bases and leading dimensions allow them.  Indices are not checked. */
int bcx_gather_rows(void* stream, const void* Z_dev, int64_t ldz, int32_t C, const void* rows_dev, int64_t n_rows,
                    void* out_dev, int64_t ldo);
/* Closed-form column sums of the linear-regression family (family 2) from the one-time second moments of the data:
 *   sum_n (y_n - x_n.theta)^2 = yy - 2 theta^T X^T y + theta^T X^T X theta
 * so the 1 + opt_itrs full-data column sums of a SparseVI step (sparsevi.py:23-42, 69-76; model_linreg.py:4-10) cost
 * O(S D^2) each instead of a 2 N D S projection.
 *   bcx_project_moments        M_dev (C x ldm doubles, both triangles) = Z^T Z over the N rows of Z_dev (N x ldz, C <= 1024
 *                              columns used: the D features and the response); fp64 MFMA, fixed summation order;
 *                              work_dev: bcx_project_moments_scratch_bytes(N, C) bytes.  Row shards: sum the M of the shards.
 *   bcx_project_colsum_moments colsum_dev[s] = sum_n vecs[n][s] (centred over s, as bcx_project_colsum returns it) for the
 *                              data whose moments are M_dev (features in [0, D), response at ycol): thetabar, then
 *                              Delta G on the fp64 matrix cores; work_dev: bcx_project_colsum_moments_scratch_bytes(D, S)
 *                              bytes, ZERO before the first call (every call leaves them zero: a zero word is a partial
 *                              sum that has not been written yet). */
int64_t bcx_project_moments_scratch_bytes(int64_t N, int32_t C);
int64_t bcx_project_colsum_moments_scratch_bytes(int32_t D, int32_t S);
int bcx_project_moments(void* stream, const void* Z_dev, int64_t N, int64_t ldz, int32_t C, void* M_dev, int64_t ldm,
                        void* work_dev, int64_t work_bytes);
int bcx_project_colsum_moments(void* stream, const void* M_dev, int64_t ldm, int32_t D, int32_t ycol,
                               const void* theta_dev, int32_t S, int32_t ldt, double sigsq, void* colsum_dev, void* work_dev);
/* ... expanded around a point the caller supplies: tbar_dev = D doubles near the draws (the expansion is exact around any
 * point; bcx_linreg_posterior_draw leaves the mean of its draws), NULL = bcx_project_colsum_moments. */
int bcx_project_colsum_moments_at(void* stream, const void* M_dev, int64_t ldm, int32_t D, int32_t ycol,
                                  const void* theta_dev, int32_t S, int32_t ldt, double sigsq, void* colsum_dev, void* work_dev,
                                  const void* tbar_dev);
/* The two projections SparseVI's weight optimisation needs at every ADAM step (sparsevi.py:35-41 at fresh draws), for the
 * linear-regression family with the data's column sums in closed form: bcx_project_colsum_moments_at (M_dev, ldm, ycol_m,
 * colsum_dev, work_dev, tbar_dev: as there, tbar_dev given) and bcx_project_write_points of the Nc coreset points Zc_dev with
 * center = 0 (out_dev: Nc x ldo raw log-likelihoods) -- as ONE launch when the points take the 32 x 32-block kernel (both
 * only read the draws), else as the two calls.  Same results bit for bit either way. */
int bcx_project_points_colsum_moments(void* stream, const void* Zc_dev, int64_t Nc, int64_t ldzc, int32_t D, int32_t ycol,
                                      const void* theta_dev, int32_t S, int32_t ldt, double sigsq, void* out_dev, int64_t ldo,
                                      const void* M_dev, int64_t ldm, int32_t ycol_m, void* colsum_dev, void* work_dev,
                                      const void* tbar_dev);
/* SparseVI's weight optimisation with the weights resident on the device (sparsevi.py:69-76 -> util/opt.py:4-28): the
 * reference's loop body is projector.update(w, pts) [sampler call, sparsevi.py:25], two projections [sparsevi.py:35-41],
 * the gradient [sparsevi.py:72-74] and one projected-ADAM update [opt.py:19-25]; with these two entry points and the
 * projection calls above a host enqueues opt_itrs such steps and reads the k weights back once (csrc/svi.hip).
 *   bcx_linreg_posterior_draw  theta_dev (S x ld) = S draws from the posterior of the weighted coreset under the Gaussian
 *                              linear-regression model with a N(mu0, Sig0) prior (the sampler of the reference's
 *                              examples/linear_regression/main.py:124-147), theta = mu_w + R_dev Uw^T for the standard-normal
 *                              R_dev (S x ld, 16-byte aligned), as a rank-k correction of the prior's factor Sig0 = U0 U0^T
 *                              through a k x k Cholesky; tbar_dev (D) = the mean of the draws, formed as the "draw" of
 *                              Rbar_dev (ld doubles: the column means of R_dev, supplied by the caller).  Per-point inputs (formed
 *                              by the caller when the points change): K0 = (X U0)(X U0)^T (k x k), xmu0 = X mu0, y (k),
 *                              XU0 = X U0 and XS0 = X Sig0 (k x ld); per-model: U0T = U0^T (D x ld), mu0 (D).  w_dev: the
 *                              k weights (negative entries count as 0).  k <= 64, ld even.
 *   bcx_sparsevi_adam_step     resid = scaling colsum - w corevecs, g = -corevecs resid / S, then opt.py:19-25 on w_dev /
 *                              mom1_dev / mom2_dev (k doubles each) with every weight clamped at 0 (nn_idcs = None).
 *                              core_dev: k x ldc projected coreset points (core_is_raw != 0: as bcx_project_write_raw leaves
 *                              them -- the row means of projector.py:21 are then taken here); sched_dev: 3 doubles per step -- step_sched(i),
 *                              1 - b1^(i+1), 1 - b2^(i+1), evaluated by the host; step: i; trace_dev: NULL or steps x k
 *                              doubles receiving the weights after each step.
 * Asynchronous on `stream`; errors: bcx_project_last_error(). */
int bcx_linreg_posterior_draw(void* stream, int32_t k, int32_t D, int32_t ld, const void* w_dev, const void* K0_dev,
                              const void* xmu0_dev, const void* y_dev, const void* XU0_dev, const void* XS0_dev,
                              const void* U0T_dev, const void* mu0_dev, double sigsq, const void* R_dev, const void* Rbar_dev,
                              int32_t S, void* theta_dev, void* tbar_dev);
/*   bcx_linreg_posterior_apply the same draws for a loop of calls at the same points: G_dev (S x ld) = R U0^T and Gbar_dev (ld, its
 *                              column means) are formed once for all steps (bcx_linreg_posterior_draw with k = 0 and a zero
 *                              prior mean returns R U0^T), a step is then the rank-k correction theta = mu_w + G - (G X^T) B2
 *                              of rows read once.  X_dev: the points' features (k x ld, padding 0).  gscale_dev (ld doubles,
 *                              or NULL): the prior's factor is diag(gscale) (an isotropic / diagonal prior) and G_dev / Gbar_dev
 *                              hold R and its column means themselves -- the scaling is applied as the rows are read, R U0^T
 *                              is never stored.  Serves the (k, ld) for which bcx_linreg_posterior_apply_ok is non-zero
 *                              (k <= 32 and 16 k ld <= 128 KiB of LDS). */
int bcx_linreg_posterior_apply_ok(int32_t k, int32_t ld);
int bcx_linreg_posterior_apply(void* stream, int32_t k, int32_t D, int32_t ld, const void* w_dev, const void* K0_dev,
                               const void* xmu0_dev, const void* y_dev, const void* X_dev, const void* XS0_dev,
                               const void* mu0_dev, double sigsq, const void* G_dev, const void* Gbar_dev, int32_t S,
                               void* theta_dev, void* tbar_dev, const void* gscale_dev);
int bcx_sparsevi_adam_step(void* stream, int32_t k, int32_t S, const void* colsum_dev, double scaling, const void* core_dev,
                           int64_t ldc, void* w_dev, void* mom1_dev, void* mom2_dev, const void* sched_dev, int32_t step,
                           double b1, double b2, double eps, void* trace_dev, int32_t core_is_raw);
/* The sampler's raw material without the framework: bcx_standard_normal fills out_dev with `count` standard normal doubles
 * (counter-based Philox-4x32-10 + Box-Muller: the numbers of pair counters offset .. offset + ceil(count / 2) - 1 under the key
 * `seed`, the same whatever the launch shape; a caller that advances `offset` by ceil(count / 2) per call draws one
 * reproducible stream -- the role of np.random.randn in examples/linear_regression/main.py:147); bcx_column_means writes the
 * column means of `nblocks` blocks of n x ld doubles (block_stride doubles apart) to out_dev[b * out_stride + c] -- the means
 * of every ADAM step's normal numbers in one launch (their image under the posterior's factor is the mean of the draws). */
int bcx_standard_normal(void* stream, uint64_t seed, uint64_t offset, int64_t count, void* out_dev);
int bcx_column_means(void* stream, const void* rows_dev, int32_t nblocks, int32_t n, int32_t ld, int64_t block_stride,
                     void* out_dev, int64_t out_stride);
/* The same ADAM step for up to 4096 weights: up to 16 the single-workgroup kernel above, beyond it two launches of one
 * workgroup per slab of 8 weights (row means + the slabs' shares of w.dot(corevecs); resid, gradient, moments, step), which
 * need work_dev = bcx_sparsevi_adam_scratch_bytes(k, S) bytes of scratch (0 for k <= 16; -1: k or S out of range). */
int64_t bcx_sparsevi_adam_scratch_bytes(int32_t k, int32_t S);
int bcx_sparsevi_adam_step_ws(void* stream, int32_t k, int32_t S, const void* colsum_dev, double scaling, const void* core_dev,
                              int64_t ldc, void* w_dev, void* mom1_dev, void* mom2_dev, const void* sched_dev, int32_t step,
                              double b1, double b2, double eps, void* trace_dev, int32_t core_is_raw, void* work_dev,
                              int64_t work_bytes);
/* One step of the quasi-Newton coreset (Naik, Rousseau and Campbell, 2022) on k device-resident weights (csrc/qn.hip).  With
 * V (k x S) the rows of core_dev centred over the S draws (core_is_raw != 0: the row means of projector.py:21 are taken here,
 * into a centred copy in scratch; 0: the rows arrive centred) and c = scaling x colsum_dev (S):
 *     resid = c - V^T w                                  (sparsevi.py:47 / :72)
 *     b     = V resid / S                                (minus SparseVI's gradient, sparsevi.py:74)
 *     G     = V V^T / S
 *     d     : (G + tau I) d = b                          (tau >= 0, absolute, in squared log-likelihood units)
 *     w     <- max(w + gamma d, 0)                       (NumPy's maximum: a NaN stays a NaN),  gamma = sched_dev[step]
 * The system is solved multiplied through by S, (V V^T + S tau I) d = V resid: V V^T on the fp64 matrix cores (the tiled
 * Gram kernel), a Cholesky factorisation -- one workgroup with the matrix in LDS up to 128 weights, beyond it panels of 32
 * columns ordered by launch boundaries (diagonal tile in one wave, panel solve, trailing update on the matrix cores) -- and
 * the two triangular solves.  No grid barrier, no wait between workgroups, no floating-point atomics, every sum in a fixed
 * order: the same inputs on the same device give the same bits.  1 <= k <= 4096, 1 <= S <= 8192, ldc >= S.
 * sched_dev: one double per step (gamma_i, evaluated by the host); dir_dev: NULL or k doubles receiving d; trace_dev: NULL or
 * steps x k doubles, row `step` receiving the weights after this step; status_dev: one int32 the caller zeroes when a loop of
 * steps starts and reads once after it -- a step raises it to 1 (max: it is never cleared here) when a pivot is not positive
 * or NaN, and while it is non-zero, in that step and every later one, w_dev and dir_dev are left untouched.  work_dev:
 * bcx_quasi_newton_scratch_bytes(k, S) bytes (-1: k or S out of range), 16-byte aligned, owned by the call until it has
 * completed.  Asynchronous on `stream`; errors: bcx_project_last_error(). */
int64_t bcx_quasi_newton_scratch_bytes(int32_t k, int32_t S);
int bcx_quasi_newton_step(void* stream, int32_t k, int32_t S, const void* colsum_dev, double scaling, const void* core_dev,
                          int64_t ldc, int32_t core_is_raw, void* w_dev, const void* sched_dev, int32_t step, double tau,
                          void* dir_dev, void* trace_dev, void* status_dev, void* work_dev, int64_t work_bytes);
/* The weighted conjugate posterior of Gaussian linear regression for ANY number of weighted points, in the reference's own
 * arithmetic (examples/common/model_linreg.py:26-41 weighted_post returns mup, USigp, LSigpInv; the sampler of
 * examples/linear_regression/main.py:141-147 draws muw + randn . USigw^T):
 *     P = S0inv + X^T diag(max(w, 0)) X / sigsq = L L^T,   U_dev (D x ldu doubles, row-major, UPPER triangular) = USigp = L^-T,
 *     u_dev (D) = L^-1 (rhs0 + X^T (w y) / sigsq),  rhs0 = Sig0^-1 mu0,   mu_dev (D, may be NULL) = mup = U u,
 * from k weights w_dev that live on the device (SparseVI's ADAM loop updates them there), the points' features BY points
 * XT_dev (D x ldx: row a holds feature a of the k points; ldx >= k rounded up to 32, the padding zero, 16-byte aligned), their
 * responses y_dev and the prior precision S0inv_dev (D x lds0).  D <= 1024, k <= 4096; U_dev's lower triangle is never
 * written (zero it once), ldu even; work_dev: bcx_linreg_posterior_factor_scratch_bytes(D) bytes, 16-byte aligned, not
 * shared between streams.  Asynchronous on `stream`: P on the fp64 matrix cores, then ONE cooperative launch of <= 63
 * workgroups (blocked Cholesky whose row operations also produce L^-T and L^-1 rhs: csrc/lrpost.hip), then -- only when
 * mu_dev is given -- the product U u; the cooperative launch's workgroups hand tiles to each other and give up a wait after
 * 2 s.  work_dev holds a status word, the worst outcome of every factorisation since bcx_linreg_posterior_factor_clear_status
 * (enqueued on `stream`; call it once before the first factorisation a status read is to cover -- a whole loop of them, or one
 * call).  bcx_linreg_posterior_factor_status synchronises the stream and returns BCX_ERR_TIMEOUT if a wait expired, BCX_ERR_STATE
 * if a pivot was not positive or NaN (NaN / non-finite weights or points: the weights are clamped by max(w, 0) with NumPy's
 * rule, which keeps a NaN), BCX_OK otherwise; reading does not clear the word.  Where the reference would go on with NaN
 * weights, the SparseVI loops of the package raise on this status (an error instead of NaN weights).
 * bcx_linreg_posterior_draw_factored: theta_dev (S x ld) = mup + R U^T = (R + 1 u^T) U^T for standard-normal R_dev (S x ld,
 * 16-byte aligned rows), tbar_dev (D) = mup + Rbar U^T for their column means Rbar_dev (ld) -- the mean of the draws. */
int64_t bcx_linreg_posterior_factor_scratch_bytes(int32_t D);
int bcx_linreg_posterior_factor(void* stream, int32_t k, int32_t D, int32_t ldx, const void* w_dev, const void* XT_dev,
                                const void* y_dev, const void* S0inv_dev, int32_t lds0, const void* rhs0_dev, double sigsq,
                                void* work_dev, int64_t work_bytes, void* U_dev, int64_t ldu, void* u_dev, void* mu_dev);
int bcx_linreg_posterior_factor_clear_status(void* stream, int32_t D, void* work_dev);
int bcx_linreg_posterior_factor_status(void* stream, int32_t D, const void* work_dev);
int bcx_linreg_posterior_draw_factored(void* stream, int32_t D, int32_t ld, const void* U_dev, int64_t ldu, const void* u_dev,
                                       const void* R_dev, const void* Rbar_dev, int32_t S, void* theta_dev, void* tbar_dev);
/* The sampler of the reference's logistic / Poisson regression experiment (examples/logistic_poisson_regression/main.py:15-41
 * get_laplace, :155-162 sampler_w) from k weights that live on the device: the Laplace approximation of the weighted posterior
 * of the points pts_dev (k x ldp; logistic: rows y x of D values; Poisson: rows [x, y]) under a standard-normal prior --
 * mu_dev (D) = the mode (damped Newton to |step| < tol, at most max_iter steps; warm != 0: started from the contents of mu_dev,
 * e.g. the previous ADAM step's mode), and the draws theta_dev (S x ld) = mu + R W, tbar_dev (D) = mu + Rbar W with W = L^-1 for
 * the Cholesky factor L of the negative Hessian at the mode (Sigma = W^T W), R_dev (S x ld) standard normal numbers and Rbar_dev
 * their column means.  family 0: logistic, 1: Poisson (softplus rate).  ONE launch of one workgroup (csrc/laplace.hip), the
 * points resident in LDS: serves the (k, D) for which bcx_laplace_sampler_ok is non-zero (D <= 32, the points + four doubles
 * each within 96 KiB).  status_dev (3 int32): [0] 0 converged / 1 iteration limit / 2 no positive definite Newton matrix (NaN
 * weights included: they are clamped by max(w, 0) with NumPy's rule, which keeps a NaN), [1] Newton steps taken, [2] the
 * worst [0] since the caller zeroed it (max over calls: a loop of calls reads it once).  Asynchronous on `stream`. */
int bcx_laplace_sampler_ok(int32_t k, int32_t D);
int64_t bcx_laplace_sampler_lds_bytes(int32_t k, int32_t D);
int bcx_laplace_sampler(void* stream, int32_t family, int32_t k, int32_t D, const void* w_dev, const void* pts_dev, int64_t ldp,
                        void* mu_dev, int32_t warm, double tol, int32_t max_iter, const void* R_dev, const void* Rbar_dev,
                        int32_t S, int32_t ld, void* theta_dev, void* tbar_dev, void* status_dev);
/* The same fit and draws for ANY k (the points beyond bcx_laplace_sampler_ok, the resident full data set): the points stay in
 * device memory and are streamed by up to one workgroup per CU in ONE persistent launch (csrc/laplace_stream.hip); per pass
 * every workgroup writes one record of partial sums, the records are added in workgroup order after a grid barrier (no
 * floating-point atomics: a fit is bit-reproducible for a given (k, D) on a given device) and every workgroup takes the
 * Newton step of bcx_laplace_sampler itself.  Same arguments, outputs and status word; status [0] / [2] = 3: a wait between
 * the workgroups expired (GPU shared / preempted), the outputs are not valid.  work_dev: bcx_laplace_stream_scratch_bytes(k, D)
 * bytes (-1: bad k / D), owned by the call until it has completed.  BCX_ERR_STATE when the device cannot hold the launch's
 * workgroups together.  Asynchronous on `stream`. */
int64_t bcx_laplace_stream_scratch_bytes(int32_t k, int32_t D);
int bcx_laplace_sampler_stream(void* stream, int32_t family, int32_t k, int32_t D, const void* w_dev, const void* pts_dev, int64_t ldp,
                               void* mu_dev, int32_t warm, double tol, int32_t max_iter, const void* R_dev, const void* Rbar_dev,
                               int32_t S, int32_t ld, void* theta_dev, void* tbar_dev, void* status_dev, void* work_dev,
                               int64_t work_bytes);
/* The dense re-weight's Gram matrix as an operator of its own (optimize() forms it over the active rows, snnls.py:82-97:
 * `nnls(A[:, active], b)` solves the normal equations of that k-column block): G_dev (k x ldg doubles, both triangles) =
 * V V^T for the k rows of d doubles at rows_dev (row stride ld >= d), on the fp64 matrix cores; the d products of an entry
 * are summed in a fixed order for a given (k, d) on a given device (csrc/gram.hip: tiles of G cut into equal ranges of
 * 16-value stages over the resident workgroups, partial tiles added by the workgroup that finishes the tile; rows that are
 * not 16-byte aligned and k < 192: 64 x 64 blocks, slices of the row length added in slice order), G is symmetric bit for
 * bit.  Asynchronous on `stream`.  k <= BCX_GRAM_MAX_ROWS; work_dev: bcx_gram_scratch_bytes(k, d) bytes (up to one 128 x 128
 * tile of doubles per resident workgroup).  Errors: bcx_project_last_error(). */
#define BCX_GRAM_MAX_ROWS 16384
int64_t bcx_gram_scratch_bytes(int32_t k, int32_t d);
int bcx_gram(void* stream, const void* rows_dev, int32_t k, int32_t d, int64_t ld, void* G_dev, int64_t ldg,
             void* work_dev, int64_t work_bytes);
/* bcx_gram is asynchronous; the kernel that balances the tiles over the chip hands partial tiles between workgroups and
 * gives up a wait after 5 s (a GPU shared with another process, preemption).  bcx_gram_check synchronises `stream` and
 * returns BCX_ERR_TIMEOUT if a call of this process that used the scratch `work_dev` gave up -- that call's G is
 * not valid (zero the first 8 bytes of the scratch to re-arm); BCX_OK otherwise.  optimize() (bcx_optimize) makes the same
 * check on its own Gram launches and returns BCX_ERR_TIMEOUT. */
int bcx_gram_check(void* stream, const void* work_dev);
/* Two row passes of the constructor path behind a device projector (reference: projector.py:21, hilbert.py:19-22):
 * bcx_center_rows subtracts every row's mean in place (rows_dev: N x ld doubles, S used per row); bcx_row_sumsq writes every
 * row's sum of squares to out_dev (N doubles) -- the subsample branch drops the rows where it is zero. */
int bcx_center_rows(void* stream, void* rows_dev, int64_t N, int32_t S, int64_t ld);
int bcx_row_sumsq(void* stream, const void* rows_dev, int64_t N, int32_t S, int64_t ld, void* out_dev);
/* The text of the calling host thread's last failure in an entry point that takes no bcx_solver* (projection, moments, Gram,
 * PSVI, SVI, quasi-Newton, Gaussian, linear-regression posterior, Laplace, HMC, NUTS, predictive, pair statistics):
 * "<entry point>: <what>", and for BCX_ERR_HIP "<entry point>: <the HIP call>: <HIP's reason>".  One string per thread: "" before
 * that thread's first failure, valid and unchanged until its next one; a call that succeeds leaves it alone. */
const char* bcx_project_last_error(void);
/* Measurement: hipEvents around the projection kernel alone, recorded on the stream the kernel is launched on.
 * bcx_project_profile(1) starts timing every later projection launch of the calling host thread, (0) stops;
 * bcx_project_profile_read returns the totals since the start: kernel milliseconds, launches, and the algorithmic
 * flops 2 N D S of those launches (the roofline figure of bench.py --config c5 / c3). */
int bcx_project_profile(int32_t on);
int bcx_project_profile_read(double* ms_total, int64_t* launches, double* flops);
/* ---- BatchPSVI: gradients of the projection with respect to the pseudo-points (csrc/psvi.hip) ----
 * The rows P_dev (k x ldp doubles: the D features first; for family 1 / 2 the response in column ycol) are pseudo-points,
 * theta_dev (S x ldt) the current samples, family / param as for bcx_project_write.  Every family's gradient of a point's
 * log-likelihood is c(i, s) times theta_s (family 2: [theta_s, 1], so dz = D + 1; otherwise dz = D), see csrc/psvi.hip.
 * Limits: 1 <= k <= BCX_PSVI_MAX_POINTS, 1 <= S <= BCX_PSVI_MAX_SAMPLES, 1 <= D <= BCX_PSVI_MAX_DIM; outside them an
 * entry returns BCX_ERR_ARG with a message in bcx_project_last_error().  Asynchronous on `stream`; deterministic (fixed
 * reduction orders, no atomics).  work_dev: bcx_psvi_gradient_scratch_bytes(k, S) bytes (-1: outside the limits). */
#define BCX_PSVI_MAX_POINTS 4096
#define BCX_PSVI_MAX_SAMPLES 8192
#define BCX_PSVI_MAX_DIM 1024
int64_t bcx_psvi_gradient_scratch_bytes(int32_t k, int32_t S);
/* glls_dev (k x S x dz, row-major) = the gradient projection of the reference's project(pts, grad=True)
 * (bayesiancoresets/projector.py:25-27: centred over the LAST axis, the coordinates of the point) with the family gradients
 * of examples/common/model_lr.py:50-57, model_linreg.py:12-17 and model_poiss.py:58-67 (the intended c(i, s) theta_s). */
int bcx_project_grad_points(void* stream, int32_t family, const void* P_dev, int32_t k, int64_t ldp, int32_t D, int32_t ycol,
                            const void* theta_dev, int32_t S, int32_t ldt, double param, void* glls_dev, void* work_dev);
/* One gradient evaluation of BatchPSVI (bayesiancoresets/coreset/bpsvi.py:47-55) from colsum_dev (S: the data's centred
 * column sums, sum_n vecs[n]), corevecs_dev (k x ldcv: the centred projections of the pseudo-points, bcx_project_write_points
 * with center = 1), w_dev (k weights) and scaling:  out_dev = [resid (S) | wgrad (k) | ugrad (k x dz)] with
 *   resid = scaling colsum - w^T corevecs,  wgrad = -corevecs resid / S,  ugrad[i] = -(w_i / S) sum_s glls[i, s, :] resid[s]
 * -- the k x S x dz gradients are never formed (two products on the fp64 matrix cores). */
int bcx_psvi_gradient(void* stream, int32_t family, const void* P_dev, int32_t k, int64_t ldp, int32_t D, int32_t ycol,
                      const void* theta_dev, int32_t S, int32_t ldt, double param, const void* colsum_dev, const void* corevecs_dev,
                      int64_t ldcv, const void* w_dev, double scaling, void* out_dev, void* work_dev);
/* ---- The Gaussian-mean family (family id 3; reference: examples/common/model_gaussian.py; csrc/gauss.hip) ----
 * Rows are the points x (N x D, no response column), Siginv the inverse of the known likelihood covariance.  With tbar the mean
 * of the draws the centred log-likelihoods are linear in x: vecs[n, s] = x_n . g_s + bias_s - (row mean),
 * g_s = Siginv (theta_s - tbar), bias_s = -(tbar + (theta_s - tbar) / 2) . g_s.  The projection entry points above take family 3
 * with ycol ignored and theta_dev = the S x (D + 1) OPERAND [g_s | bias_s] (ldt >= D + 1; `param` unused); values omit what is
 * constant along a row (it cancels in every centred result).  bcx_project_points_colsum_moments, bcx_project_grad_points and
 * bcx_psvi_gradient refuse family 3 (BCX_ERR_ARG).
 * bcx_gaussian_operand: out_dev (n x ldo, ldo >= D + 1) = Siginv (row - tbar) in columns [0, D) for the n rows of rows_dev, and in
 * column D  mode 0: the bias above (rows are draws)   mode 1: the mean of the D coordinates (rows are points: the gradient entries).
 * Siginv_dev: D x D symmetric (leading dimension ldsig) or NULL = identity.  tbar_dev NULL: the mean of the rows themselves, formed
 * in work_dev (D doubles).  D <= 4096. */
int bcx_gaussian_operand(void* stream, const void* rows_dev, int32_t n, int64_t ldx, int32_t D, const void* Siginv_dev, int64_t ldsig,
                         const void* tbar_dev, void* out_dev, int64_t ldo, int32_t mode, void* work_dev);
/* xsum_dev (D) = sum_n x_n in one fixed order; work_dev: bcx_gaussian_first_moment_scratch_bytes(N, D) bytes. */
int64_t bcx_gaussian_first_moment_scratch_bytes(int64_t N, int32_t D);
int bcx_gaussian_first_moment(void* stream, const void* Z_dev, int64_t N, int64_t ldz, int32_t D, void* xsum_dev, void* work_dev,
                              int64_t work_bytes);
/* The centred column sums of the projected data in closed form: colsum_dev[s] = xsum . g_s + n_rows bias_s, minus the mean over s. */
int bcx_gaussian_colsum_moments(void* stream, const void* xsum_dev, double n_rows, int32_t D, const void* operand_dev, int32_t S,
                                int64_t ldt, void* colsum_dev);
/* S draws of the weighted posterior (model_gaussian.py:23-30): precision Sig0inv + (sum w) Siginv.  The caller forms once
 * Siginv = L L', L^-1 Sig0inv L^-T = V diag(lam) V', W = L^-T V (W_dev, WT_dev: D x D row-major and its transpose), c0 = Sig0inv mu0.
 * theta_dev (S x ld) = mu_w + (R scale) W', scale = (lam + sum w)^-1/2, R_dev (S x ld) normal numbers, Rbar_dev (ld) their column
 * means; tbar_dev (D) = the mean of the draws.  w_dev / pts_dev (k x ldp) are read from device memory (k = 0: the prior).
 * state_dev: 2 D doubles of scratch.  status_dev (int32): set to 1 when some lam + sum w is not positive (NaN weights included);
 * never cleared by the library.  D <= 1024. */
int bcx_gaussian_posterior_draw(void* stream, int32_t k, int32_t D, const void* w_dev, const void* pts_dev, int64_t ldp,
                                const void* c0_dev, const void* Siginv_dev, const void* W_dev, const void* WT_dev, const void* lam_dev,
                                const void* R_dev, const void* Rbar_dev, int32_t S, int32_t ld, void* theta_dev, void* tbar_dev,
                                void* state_dev, void* status_dev);
/* The two BatchPSVI entries for family 3 (csrc/psvi.hip): operand_dev as above, H_dev (k x ldh) = bcx_gaussian_operand(points,
 * mode 1) at the same tbar.  glls_dev: k x S x D.  out_dev / work_dev / limits as for bcx_psvi_gradient (dz = D). */
int bcx_project_grad_points_gaussian(void* stream, const void* operand_dev, int32_t S, int64_t ldt, int32_t D, const void* H_dev,
                                     int32_t k, int64_t ldh, void* glls_dev, void* work_dev);
int bcx_psvi_gradient_gaussian(void* stream, const void* operand_dev, int32_t S, int64_t ldt, int32_t D, const void* H_dev, int32_t k,
                               int64_t ldh, const void* colsum_dev, const void* corevecs_dev, int64_t ldcv, const void* w_dev,
                               double scaling, void* out_dev, void* work_dev);
/* One ADAM step of BatchPSVI's device-resident loop (csrc/psvi.hip psvi_adam_kernel): the reference's nn_opt
 * (bayesiancoresets/util/opt.py:15-23) on the state x = [w (k) | P (k x d)] with nn_idcs = arange(k) (coreset/bpsvi.py:57-60: only
 * the weights are clamped at 0, by NumPy's rule, which keeps a NaN):
 *     m1 = b1 m1 + (1 - b1) g,  m2 = b2 m2 + (1 - b2) g^2,  x -= sched[3 i] m1 / sched[3 i + 1] / (eps + sqrt(m2 / sched[3 i + 2]))
 * grad_dev: the out_dev of bcx_psvi_gradient[_gaussian] as it stands, [resid (S) | wgrad (k) | ugrad (k x d)] (d is the gradient's
 * dz: a caller whose points have another column count has no step to take).  w_dev: k weights; P_dev: the points, k x ldp, ldp
 * even and P_dev 16-byte aligned (what the projection / gradient entries read); mom1_dev / mom2_dev: laid out as the state is,
 * [k doubles, padded to an even count | k x ldp], 16-byte aligned, zero before step 0.  sched_dev / step: as bcx_sparsevi_adam_step.
 * XT_dev / y_dev (both or neither): a second copy of the new points in the form bcx_linreg_posterior_factor reads -- features BY
 * points (XT: (d - 1) x ldk, ldk >= k rounded up to 32; entries beyond column k are never written, so padding that is zero stays
 * zero) and the last column as y (k) -- written by the same launch, the same bits.  trace_dev: NULL or steps x k (1 + d) doubles
 * receiving [w | P (k x d, dense)] after each step.  1 <= k <= BCX_PSVI_MAX_POINTS, 1 <= d <= BCX_PSVI_ADAM_MAX_COLS,
 * 1 <= S <= BCX_PSVI_MAX_SAMPLES; BCX_ERR_ARG otherwise.  One launch, elementwise, no atomics; asynchronous on `stream`. */
#define BCX_PSVI_ADAM_MAX_COLS 4096
int bcx_psvi_adam_step(void* stream, int32_t k, int32_t d, const void* grad_dev, int32_t S, void* w_dev, void* P_dev, int64_t ldp,
                       void* mom1_dev, void* mom2_dev, const void* sched_dev, int32_t step, double b1, double b2, double eps,
                       void* XT_dev, int64_t ldk, void* y_dev, void* trace_dev);
/* The weighted log joint of the logistic / Poisson regression models and its gradient for C parameter vectors at once
 * (examples/common/model_lr.py:34-39, 59-64; model_poiss.py:40-46, 69-74, prior constant and the Poisson -log y! included):
 *     value_dev[c] = sum_j w_j log p(z_j | theta_c) - |theta_c|^2 / 2 - D/2 log 2 pi,   grad_dev[c] (row stride ldt) its gradient.
 * Z_dev: N x ldz rows as bcx_laplace_sampler reads them (logistic y x, Poisson [x, y]); w_dev: N weights or NULL (ones);
 * Theta_dev: C x ldt.  Any N >= 0 and C >= 1, D <= 32.  work_dev: bcx_log_joint_grad_scratch_bytes(N, D, C) bytes (-1: out of
 * range).  Per-workgroup partial sums in a fixed order and a fixed-order second level (csrc/hmc.hip), no floating-point
 * atomics: the same inputs give the same bits.  Asynchronous on `stream`. */
int64_t bcx_log_joint_grad_scratch_bytes(int64_t N, int32_t D, int32_t C);
int bcx_log_joint_grad(void* stream, int32_t family, const void* Z_dev, int64_t N, int64_t ldz, int32_t D, const void* w_dev,
                       const void* Theta_dev, int32_t C, int32_t ldt, void* value_dev, void* grad_dev, void* work_dev);
/* Hamiltonian Monte Carlo on the weighted posterior of k points -- the evaluation of the reference's logistic / Poisson
 * experiment (examples/logistic_poisson_regression/main.py:107-127, 205-232 and examples/common/mcmc.py:60-70 run Stan with
 * 'w': wts; this is HMC with a fixed number of leapfrog steps, not NUTS).  `chains` chains move in xi with theta = mu + W^T xi
 * (mu_dev: D or NULL = 0; W_dev: D x D, row stride ldw, or NULL = identity), unit mass matrix, from xi = 0, for n_warmup +
 * n_samples = T transitions.  Transition t of chain c reads the D + 3 standard normals noise_dev[(c T + t)(D + 3) ..]: D momenta,
 * two for the accept threshold e = (z1^2 + z2^2) / 2 (accept iff dH <= e), one for the step jitter eps_t = eps exp(0.1 z).  The
 * warm-up adapts eps per chain from eps0 by dual averaging (Hoffman & Gelman 2014, Alg. 5: delta 0.8, gamma 0.05, t0 10,
 * kappa 0.75); sampling uses the averaged step.  fixed_eps > 0 (a development argument): that base step throughout, no adaptation.
 * Outputs: samples_dev (chains x T x ld, theta after every transition, warm-up included); xi_dev / prop_dev (the same shape, or
 * NULL: the states and the proposals in xi); diag_dev (chains x T x 6: dH, accepted, eps_t, the next transition's base step,
 * the dual-averaging Hbar and log eps-bar); accept_dev (chains: the accept rate of the sampling transitions); eps_dev (chains:
 * their base step); status_dev (2 int32): [0] of this call 0 ok / 1 a non-finite dH was rejected / 2 the log joint at the start
 * is not finite (NaN weights or points: nothing is scrubbed), [1] the worst [0] since the caller zeroed it.
 * bcx_hmc_coreset: ONE launch, a workgroup per chain, the points in LDS -- the (k, D) for which bcx_hmc_coreset_ok is non-zero
 * (D <= 32, bcx_hmc_coreset_lds_bytes within the LDS the device gives a workgroup less the kernel's own).
 * bcx_hmc_stream: any N (the full data set), at most 256 chains: every leapfrog step is one bcx_log_joint_grad-shaped pass over
 * the rows for all chains and a small kernel per chain; enqueued on `stream` without host synchronisation; work_dev:
 * bcx_hmc_stream_scratch_bytes(N, D, chains) bytes.  The two run the same transition text and agree to rounding. */
int bcx_hmc_coreset_ok(int32_t k, int32_t D);
int64_t bcx_hmc_coreset_lds_bytes(int32_t k, int32_t D);
int bcx_hmc_coreset(void* stream, int32_t family, int32_t k, int32_t D, const void* w_dev, const void* pts_dev, int64_t ldp,
                    const void* mu_dev, const void* W_dev, int64_t ldw, int32_t chains, int32_t n_warmup, int32_t n_samples,
                    int32_t leapfrog, double eps0, double fixed_eps, const void* noise_dev, int32_t ld, void* samples_dev,
                    void* xi_dev, void* prop_dev, void* diag_dev, void* accept_dev, void* eps_dev, void* status_dev);
int64_t bcx_hmc_stream_scratch_bytes(int64_t N, int32_t D, int32_t chains);
int bcx_hmc_stream(void* stream, int32_t family, int64_t N, int32_t D, const void* w_dev, const void* Z_dev, int64_t ldz,
                   const void* mu_dev, const void* W_dev, int64_t ldw, int32_t chains, int32_t n_warmup, int32_t n_samples,
                   int32_t leapfrog, double eps0, double fixed_eps, const void* noise_dev, int32_t ld, void* samples_dev,
                   void* xi_dev, void* prop_dev, void* diag_dev, void* accept_dev, void* eps_dev, void* status_dev, void* work_dev,
                   int64_t work_bytes);
/* One iteration's chain half of Coreset MCMC (Chen & Campbell 2024; csrc/hmc.hip cmc_advance_kernel): `chains`
 * chains (at most 8192) that live across calls in state_dev (bcx_cmc_state_bytes(chains) bytes; fresh != 0: they start from
 * xi = 0, base step eps0) each take `thin` transitions of bcx_hmc_coreset at the weights w_dev holds NOW -- the target and its
 * gradient at the carried state are evaluated again first -- with the k points in LDS (1 <= k <= 4096 within bcx_cmc_advance_ok).
 * first_transition is the index of the call's first transition in the chains' life: the transitions with index below
 * n_adapt_transitions adapt the step by the dual averaging with that index, the last of them hands over exp(log eps-bar), later
 * ones keep it.  noise_dev, samples_dev, xi_dev, prop_dev (the last two may be NULL) and diag_dev are this call's chains x thin x
 * (D + 3 | ld | ld | ld | 6) blocks, laid out and filled as bcx_hmc_coreset's.  Then, with theta_c the chains' states:
 *     core_dev[m ldc + c] = log p(z_m | theta_c) of the k points (ldc >= chains; the Poisson -log y! dropped),
 *     colsum_dev[c]       = sum_r log p(Z[rows[r]] | theta_c) - the mean of these sums over the chains (fixed order),
 * rows_dev: n_rows int64 indices into the N x ldz rows of Z_dev, or NULL with n_rows = 0: all N rows; an index outside [0, N) is
 * not read and makes its sum a NaN.  These are the core_dev (raw) / colsum_dev of bcx_sparsevi_adam_step_ws with S = chains.
 * No workgroup waits on another; a NaN is kept.  status_dev as bcx_hmc_coreset ([0] is zeroed by every call).  Asynchronous. */
int bcx_cmc_advance_ok(int32_t k, int32_t D);
int64_t bcx_cmc_advance_lds_bytes(int32_t k, int32_t D);
int64_t bcx_cmc_state_bytes(int32_t chains);
int bcx_cmc_advance(void* stream, int32_t family, int32_t k, int32_t D, const void* w_dev, const void* pts_dev, int64_t ldp,
                    const void* mu_dev, const void* W_dev, int64_t ldw, int32_t chains, int32_t thin, int32_t leapfrog, double eps0,
                    int32_t first_transition, int32_t n_adapt_transitions, int32_t fresh, const void* noise_dev, void* state_dev,
                    const void* Z_dev, int64_t N, int64_t ldz, const void* rows_dev, int64_t n_rows, void* core_dev, int64_t ldc,
                    void* colsum_dev, int32_t ld, void* samples_dev, void* xi_dev, void* prop_dev, void* diag_dev, void* status_dev);
/* The No-U-Turn sampler (Hoffman & Gelman 2014) on the same target, frame and start as bcx_hmc_coreset, for the (k, D) that fit one
 * workgroup's LDS (csrc/nuts.hip; any N: bcx_nuts_stream below): ONE launch, a workgroup per chain, no leapfrog count to choose.
 * With J = max_depth (1 .. 10), transition t of chain c reads R = D + 3 J + 2 (2^J - 1) standard normals at
 * noise_dev[(c T + t) noise_ld ..] (noise_ld >= R): D momenta; per doubling j the direction (>= 0: forward) and two for the
 * threshold e_j = (a^2 + b^2) / 2; per leaf slot 2^j - 1 + i two for e_leaf.  Doubling j takes 2^j leapfrog steps of the base
 * step (no jitter) from the right or left endpoint; a leaf with delta = H0 - H_leaf not finite or <= -1000 is a divergence; the
 * leaf replaces the doubling's proposal iff logS - delta <= e_leaf, a completed doubling the tree's iff logW - logS <= e_j; a
 * U-turn of any balanced span of the doubling discards it and stops the tree, a U-turn of the tree's endpoints stops it.  The
 * warm-up is the dual averaging of bcx_hmc_coreset on the mean of min(1, exp delta) over the transition's leaves.
 * Outputs as bcx_hmc_coreset (prop_dev: the selected state, equal to xi_dev) except diag_dev (chains x T x 8: the mean accept
 * statistic, the depth = completed doublings, the leapfrog steps, the next transition's base step, Hbar, log eps-bar, divergent
 * 0 / 1, H of the selected state - H0) and accept_dev (chains: the mean accept statistic of the sampling transitions);
 * status_dev[0]: 0 ok / 1 a leaf's energy was not finite / 2 the log joint at the start is not finite. */
int bcx_nuts_coreset_ok(int32_t k, int32_t D);
int64_t bcx_nuts_coreset_lds_bytes(int32_t k, int32_t D);
int bcx_nuts_coreset(void* stream, int32_t family, int32_t k, int32_t D, const void* w_dev, const void* pts_dev, int64_t ldp,
                     const void* mu_dev, const void* W_dev, int64_t ldw, int32_t chains, int32_t n_warmup, int32_t n_samples,
                     int32_t max_depth, double eps0, double fixed_eps, const void* noise_dev, int64_t noise_ld, int32_t ld,
                     void* samples_dev, void* xi_dev, void* prop_dev, void* diag_dev, void* accept_dev, void* eps_dev,
                     void* status_dev);
/* bcx_nuts_coreset with a metric learned in the warm-up (csrc/nuts_adapt.h).  A metric M^-1 = L L^T in the
 * coordinates xi0 of the frame passed (theta = mu + W^T xi0) is a unit metric in eta, xi0 = L eta, so the chain moves in eta with
 * the frame L^T W and the transition above; L is lower triangular, per chain, the identity at the start.
 * bcx_nuts_adapt_schedule (host only) gives the warm-up's slow windows [start, end) as `start, end` pairs in bounds (at most cap
 * pairs are written; bounds may be NULL) and returns their number (at most 32): none below 20 warm-up transitions; else init = 75,
 * term = 50, base = 25, or floor(0.15 n), floor(0.1 n) and the rest when those exceed n_warmup; windows from init, each twice as
 * long as the one before, the one whose successor would not fit before n_warmup - term extended to there.
 * After every transition of a window xi0 = L eta joins a running mean and sum of outer products (Welford).  At a window's end
 * with n draws: Sigma = n / (n + 5) S + 1e-3 * 5 / (n + 5) I (S: the sample covariance, ddof 1; metric 1 keeps its diagonal,
 * metric 2 all of it), L = chol(Sigma), eta = L^-1 xi0, the frame L^T W, the target evaluated once at the state, the accumulators
 * cleared and the dual averaging restarted from the step the ended segment averaged to (a pivot that is not positive keeps the
 * previous L).  The dual averaging runs in segments that end where a window ends and at n_warmup, each handing on exp(log
 * eps-bar).  Sampling transitions never adapt; below 20 warm-up transitions every output equals bcx_nuts_coreset's.
 * xi_dev holds eta in the frame current at that transition; at a window's last transition prop_dev holds the same state in the
 * new frame, and its diag_dev row the ended segment's Hbar and log eps-bar.  frames_dev: chains x max(windows, 1) x D x D doubles, L
 * after each window, row-major (the identity without windows); metric_dev: chains x D x D, the final L.  fixed_eps > 0 is
 * BCX_ERR_ARG; bcx_nuts_adapt_ok: the (k, D) that fit next to the adapting kernel's larger static LDS. */
int32_t bcx_nuts_adapt_schedule(int32_t n_warmup, int32_t* bounds, int32_t cap);
int bcx_nuts_adapt_ok(int32_t k, int32_t D);
int bcx_nuts_adapt(void* stream, int32_t family, int32_t k, int32_t D, const void* w_dev, const void* pts_dev, int64_t ldp,
                   const void* mu_dev, const void* W_dev, int64_t ldw, int32_t chains, int32_t n_warmup, int32_t n_samples,
                   int32_t max_depth, double eps0, double fixed_eps, const void* noise_dev, int64_t noise_ld, int32_t ld,
                   void* samples_dev, void* xi_dev, void* prop_dev, void* diag_dev, void* accept_dev, void* eps_dev,
                   void* status_dev, int32_t metric, void* frames_dev, void* metric_dev);
/* P weighted posteriors of one family, D, depth and transition counts in ONE launch of P x chains workgroups (csrc/nuts.hip
 * nuts_batch_kernel): problem p is what bcx_nuts_coreset (metric 0) or bcx_nuts_adapt (metric 1 diag / 2 dense)
 * computes for problems[p], bit for bit, with chain p chains + c in the place of chain c: noise_dev, samples_dev, xi_dev, prop_dev,
 * diag_dev, accept_dev, eps_dev, frames_dev and metric_dev are the single call's arrays with a leading dimension P, and
 * status_dev holds two words per problem ([2p] this launch, zeroed here; [2p + 1] the worst since the caller zeroed it), so a
 * start that is not finite is one problem's and the others' draws stand.  problems: a HOST array of P records; `index` is written
 * by the library (the record's place in that array), the rest as the single call's arguments (w_dev NULL: ones; mu_dev NULL: zero;
 * W_dev NULL: the identity; pts_dev may be NULL when k = 0).  table_dev: bcx_nuts_batch_table_bytes(P) bytes of device memory (-1:
 * P < 1) the records are uploaded into, in dispatch order -- k descending, so that the longest leaves start first (a heuristic
 * that was not measured); the library allocates nothing.  The launch's dynamic LDS is the largest problem's.  There is no
 * fixed_eps.  frames_dev and metric_dev are required iff metric is non-zero.  BCX_ERR_ARG: what bcx_nuts_coreset refuses, P < 1,
 * P x chains past 2^31 - 1, NULL problems or table_dev, a problem outside bcx_nuts_coreset_ok (bcx_nuts_adapt_ok with a metric),
 * a row stride below the row, ldw < D with W_dev, metric outside 0 .. 2; the message names the first bad problem. */
typedef struct bcx_nuts_problem {
  const void* w_dev;    /* k weights or NULL */
  const void* pts_dev;  /* k rows, stride ldp */
  int64_t ldp;
  const void* mu_dev;   /* D or NULL */
  const void* W_dev;    /* D x D, row stride ldw, or NULL */
  int64_t ldw;
  int32_t k;
  int32_t index;
} bcx_nuts_problem;
int64_t bcx_nuts_batch_table_bytes(int32_t P);
int bcx_nuts_batch(void* stream, int32_t family, int32_t P, const bcx_nuts_problem* problems, void* table_dev, int32_t D,
                   int32_t chains, int32_t n_warmup, int32_t n_samples, int32_t max_depth, double eps0, const void* noise_dev,
                   int64_t noise_ld, int32_t ld, void* samples_dev, void* xi_dev, void* prop_dev, void* diag_dev, void* accept_dev,
                   void* eps_dev, void* status_dev, int32_t metric, void* frames_dev, void* metric_dev);
/* The same transition, noise layout, outputs and diagnostics for any N (rows past one workgroup's LDS, the resident full data set)
 * and at most 256 chains (csrc/nuts_stream.hip): ONE persistent launch of G = max(1, min(128-row tiles of N, CUs, 256)) co-resident
 * workgroups.  A round evaluates one leaf of every chain still running: all workgroups pass over their rows for the active chains
 * and leave one partial record each, a grid barrier, the chain's owner (workgroup c mod G) adds the records in workgroup order and
 * moves the chain's NUTS state machine one leaf on, a second barrier.  No floating-point atomics: the same inputs on the same device
 * give the same bits.  Every barrier wait is bounded.  scratch_dev: bcx_nuts_stream_scratch_bytes(N, D, chains, max_depth) bytes
 * (-1: N < 0, D outside 1 .. 32, chains outside 1 .. 256, max_depth outside 1 .. 10).  BCX_ERR_STATE when the device cannot hold
 * the workgroups together.  status_dev[0]: 0 ok / 1 a leaf's energy was not finite / 2 the log joint at the start is not finite / 3
 * a barrier wait expired (the outputs are then incomplete); [1]: the worst [0] since the caller zeroed it. */
int64_t bcx_nuts_stream_scratch_bytes(int64_t N, int32_t D, int32_t chains, int32_t max_depth);
int bcx_nuts_stream(void* stream, int32_t family, int64_t N, int32_t D, const void* w_dev, const void* Z_dev, int64_t ldz,
                    const void* mu_dev, const void* W_dev, int64_t ldw, int32_t chains, int32_t n_warmup, int32_t n_samples,
                    int32_t max_depth, double eps0, double fixed_eps, const void* noise_dev, int64_t noise_ld, int32_t ld,
                    void* samples_dev, void* xi_dev, void* prop_dev, void* diag_dev, void* accept_dev, void* eps_dev,
                    void* status_dev, void* scratch_dev, int64_t scratch_bytes);
/* The log predictive density of N held-out rows under S posterior draws of the logistic / Poisson regression models
 * (csrc/predict.hip), with ll the reference's full log-likelihood (examples/common/model_lr.py:25-32;
 * model_poiss.py:25-38, the Poisson -log y! included):
 *     lppd_dev[n] = logsumexp_s ll(z_n, theta_s) - log S,      mean_dev[n] = 1/S sum_s ll(z_n, theta_s)   (mean_dev may be NULL).
 * Z_dev: N x ldz rows as bcx_log_joint_grad reads them (logistic y x, Poisson [x, y]); Theta_dev: S x ldt draws.  N >= 0, S >= 1,
 * 1 <= D <= 32.  One pass over the rows: the products on the fp64 matrix pipe, the likelihood and an online log-sum-exp (running
 * maximum, rescaled sum, sum of ll) per row in registers; the N x S table is never written.  `splits` cuts the draws into that many
 * contiguous ranges [S i / splits, S (i + 1) / splits) on different workgroups (a range may be empty), whose records are combined
 * per row in range order by a second kernel; 0: the library chooses from N, S and the device's CU count; 1 .. 4096: honoured
 * exactly.  No floating-point atomics: the same inputs, splits and device give the same bits.  A non-finite value in a row or a draw
 * makes the affected rows' outputs NaN (a row: its own; a draw: every row's); ll = -inf for some draws contributes exact zeros.
 * work_dev: bcx_log_predictive_scratch_bytes(N, D, S, splits) bytes (-1: out of range), work_bytes its size.  BCX_ERR_ARG for
 * anything else.  Asynchronous on `stream`. */
int64_t bcx_log_predictive_scratch_bytes(int64_t N, int32_t D, int64_t S, int32_t splits);
int bcx_log_predictive(void* stream, int32_t family, const void* Z_dev, int64_t N, int64_t ldz, int32_t D, const void* Theta_dev,
                       int64_t S, int64_t ldt, int32_t splits, void* lppd_dev, void* mean_dev, void* work_dev, int64_t work_bytes);
/* Sums over all pairs of two sets of draws (csrc/pairstat.hip): A_dev nA x lda against B_dev nB x ldb, D coordinates.
 *     kind 0: sum_{i,j} |a_i - b_j|_2.
 *     kind 1: sum_{i,j} k_p(a_i, b_j), the Stein kernel of the IMQ base kernel (c^2 + |x - y|^2)^(-1/2) under the scores GA_dev (nA x
 *             ldga) / GB_dev (nB x ldgb): with r = x - y and q = c^2 + |r|^2,
 *             D q^(-3/2) - 3 |r|^2 q^(-5/2) - ((g_y - g_x) . r) q^(-3/2) + (g_x . g_y) q^(-1/2).
 * B_dev = NULL: A against itself (nB, ldb, GB_dev, ldgb are not read); only the tiles on and above the diagonal are computed.
 * out_dev: 2 doubles, the total and the total of the terms i = j (0 unless kind 1 and B_dev = NULL).  1 <= nA, nB <= 2^20,
 * 1 <= D <= 32, row strides in elements >= D, c finite and > 0 for kind 1.  Differences are formed coordinate by coordinate, so equal
 * rows are at distance exactly 0.  `splits`: contiguous ranges of B's 64-row tiles per 64-row tile of A, on different workgroups
 * (0: the library chooses; 1 .. 1024: honoured exactly); one record per (tile, range) in work_dev, added in index order by a second
 * launch.  No floating-point atomics: the same arguments on the same device give the same bits.  Non-finite input is not screened:
 * it makes the total non-finite.  work_dev: bcx_pair_stat_scratch_bytes(nA, nB, D, splits) bytes (nB = 0: A against itself; -1: out
 * of range), work_bytes its size.  BCX_ERR_ARG for anything else.  Asynchronous on `stream`. */
int64_t bcx_pair_stat_scratch_bytes(int64_t nA, int64_t nB, int32_t D, int32_t splits);
int bcx_pair_stat(void* stream, int32_t kind, const void* A_dev, int64_t nA, int64_t lda, const void* GA_dev, int64_t ldga,
                  const void* B_dev, int64_t nB, int64_t ldb, const void* GB_dev, int64_t ldgb, int32_t D, double c, int32_t splits,
                  void* out_dev, void* work_dev, int64_t work_bytes);
/* Library/arch identification, e.g. "bcx 0.1 gfx950". */
const char* bcx_version(void);

#ifdef __cplusplus
}
#endif
#endif /* BCX_H */
