// qn.hip -- one step of the quasi-Newton coreset (Naik, Rousseau and Campbell, 2022) on device-resident weights.
//
// With V (k x S) the log-likelihoods of the k coreset points at the S draws, each row centred over the draws (projector.py:21),
// and c (S) = scaling x the column sums of the centred log-likelihoods of the data, a step is
//     resid = c - V^T w,   b = V resid / S,   G = V V^T / S,   (G + tau I) d = b,   w <- max(w + gamma_i d, 0)
// (NumPy's maximum: a NaN stays a NaN).  The system is solved multiplied through by S,
//     (V V^T + S tau I) d = V resid,
// so nothing is scaled: S tau is added to a diagonal entry when the factorisation loads it, and the right-hand side is V resid.
//
//   qn_center_kernel   one workgroup per slab of 8 points: row means of the raw rows, the CENTRED copy Vc (k x Sp, Sp = S rounded up
//                      to even, the padding zero -- V V^T - S m m^T would cancel for log-likelihoods like -500 +- 1), and the slab's
//                      share of V^T w (the slabbing of svi_adam_a_kernel, csrc/svi.hip; the shared pieces: slab_rows.h);
//   qn_rhs_kernel      resid from the shares added in slab order, then the slab's entries of V resid (svi_adam_b_kernel's);
//   the Gram           V V^T on the fp64 matrix cores: the tiled launch path of csrc/moments.hip / gram.hip
//                      (bcx_gram_rows_tiled: whole blocks per workgroup, slices of the row length added in slice order);
//   k <= QN_SINGLE_MAX: qn_small_kernel, ONE workgroup with the lower triangle in LDS.  The right-hand side rides along as row k
//                      of the matrix: the column operations of the right-looking Cholesky turn it into y = L^-1 (V resid), so the
//                      forward solve costs nothing; then L^T d = y by columns, and the update;
//   beyond it          a blocked right-looking Cholesky in panels of 32 columns whose stages are ordered by launch boundaries only
//                      (the precedent: warm_diag / warm_panel / warm_update, csrc/warm.hip):
//                        qn_diag_kernel    the diagonal tile and the inverse of its factor by chol32.h in one wave, and the panel's
//                                          entries of y (forward substitution on the finished tile);
//                        qn_panel_kernel   L21 = A21 L11^-T, 64 rows per workgroup;
//                        qn_update_kernel  A22 -= L21 L21^T on v_mfma_f64_16x16x4_f64, one 64 x 64 block of the lower triangle per
//                                          workgroup, and (further workgroups) the right-hand side's rows: y2 -= L21 y1;
//                      then qn_back_kernel, one workgroup: L^T d = y from the last panel to the first (the panel's inverse tile,
//                      then the panel's 32 ROWS of L against the entries left of it), and the update.
// No grid barrier, no cooperative launch, no wait on another workgroup's store, no floating-point atomics, every sum in a fixed
// order: the same inputs on the same device give the same bits.  The only atomic is the integer max on the status word.
//
// Status word (one int32, owned by the caller, zeroed when a loop starts): 1 = a pivot was not positive or NaN.  It is sticky:
// a step only ever raises it (max), and the kernel that applies the update reads it -- while it is non-zero the weights stay as
// they are, in the failing step and in every step after it.
#include <string>
#include "bcx_internal.h"
#include "dev_util.h"
#include "launch_host.h"
#include "chol32.h"
#include "slab_rows.h"

typedef double qn4d __attribute__((ext_vector_type(4)));

#define QN_KMAX 4096
#define QN_SMAX 8192
#define QN_ROWS 8            // points per slab of the two matrix-vector kernels (SVB_ROWS of csrc/svi.hip)
#define QN_NB 32             // panel width of the blocked factorisation: one chol32 tile
#define QN_UB 64             // block edge of the trailing update
#define QN_LDT (QN_UB + 8)   // [k][i] staging of the update's operands: rows 72 doubles apart (warm_gemm_kernel's layout)
#define QN_SMALL_THREADS 512
#define QN_BACK_THREADS 1024
// The single-workgroup form holds (k + 1) rows of (k + 1) doubles, the pivots and the direction in dynamic LDS and nothing
// statically: (k + 1)^2 + 2 k doubles within the 160 KiB of a CU admit k <= 140.  The threshold sits at the last whole
// panel below that bound: from 129 points on the blocked form (5+ panels) is the shorter chain of dependent steps.
#define QN_SINGLE_MAX 128
#define QN_SMALL_LDS(k) (((size_t)((k) + 1) * ((k) + 1) + 2 * (size_t)(k)) * sizeof(double))
static_assert(QN_SMALL_LDS(QN_SINGLE_MAX) <= 160 * 1024, "the single-workgroup form must fit the LDS of a CU");
static_assert(QN_SINGLE_MAX % QN_NB == 0, "the threshold is a whole number of panels");

struct QnArgs {
  const double* colsum; const double* core; const double* sched;
  double* w; double* dir; double* trace; int* status;
  double* y;           // kp: V resid, then y = L^-1 (V resid) panel by panel (entries beyond k: zero)
  double* part;        // nslab x S: the slabs' shares of V^T w
  double* Vc;          // k x Sp: centred rows
  double* G;           // kp x kp: V V^T (entries with both indices < k), then L in its lower triangle
  double* T;           // (kp / 32) x 32 x 32: inverses of the diagonal tiles of L
  double scaling, tau;
  int64_t ldc;
  int k, S, Sp, kp, step, raw_core;
};

// ---- the two matrix-vector products over the same V ----------------------------------------------------------------------------
__global__ __launch_bounds__(256) void qn_center_kernel(QnArgs a) {
  __shared__ double scm[QN_ROWS], sw[QN_ROWS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j0 = blockIdx.x * QN_ROWS, nj = min(QN_ROWS, a.k - j0);
  {
    double t[QN_ROWS / 4];                            // row means
    slab_row_sums<QN_ROWS>(a.core, a.ldc, j0, nj, a.S, a.raw_core != 0, t);
#pragma unroll
    for (int u = 0; u < QN_ROWS / 4; ++u) {
      const int q = wave + 4 * u;
      const double m = wave_allsum(t[u]) / (double)a.S;       // projector.py:21
      if (lane == 0 && q < nj) { scm[q] = m; sw[q] = a.w[j0 + q]; }
    }
  }
  __syncthreads();
  for (int s = tid; s < a.Sp; s += 256) {
    double v[QN_ROWS];
#pragma unroll
    for (int q = 0; q < QN_ROWS; ++q) v[q] = (q < nj && s < a.S) ? a.core[(size_t)(j0 + q) * a.ldc + s] - scm[q] : 0.0;
    double t = 0.0;
#pragma unroll
    for (int q = 0; q < QN_ROWS; ++q)
      if (q < nj) { a.Vc[(size_t)(j0 + q) * a.Sp + s] = v[q]; t += sw[q] * v[q]; }
    if (s < a.S) a.part[(size_t)blockIdx.x * a.S + s] = t;
  }
}

__global__ __launch_bounds__(256) void qn_rhs_kernel(QnArgs a) {
  extern __shared__ double resid[];                 // S
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j0 = blockIdx.x * QN_ROWS, nj = min(QN_ROWS, a.k - j0);
  const int nslab = (a.k + QN_ROWS - 1) / QN_ROWS;
  for (int s = tid; s < a.S; s += 256)
    resid[s] = a.scaling * a.colsum[s] - slab_share_sum(a.part, nslab, a.S, s);      // sparsevi.py:72 (shares added in slab order)
  __syncthreads();
  double g[QN_ROWS / 4];
#pragma unroll
  for (int u = 0; u < QN_ROWS / 4; ++u) {
    const int q = wave + 4 * u;
    g[u] = 0.0;
    if (q < nj) {
      const double* row = a.Vc + (size_t)(j0 + q) * a.Sp;
      for (int s = lane; s < a.S; s += 64) g[u] += row[s] * resid[s];
    }
  }
#pragma unroll
  for (int u = 0; u < QN_ROWS / 4; ++u) {
    const int q = wave + 4 * u;
    const double t = wave_allsum(g[u]);
    if (lane == 0 && q < nj) a.y[j0 + q] = t;        // V resid (the system is multiplied through by S)
  }
  if (blockIdx.x == 0)
    for (int j = a.k + tid; j < a.kp; j += 256) a.y[j] = 0.0;
}

// w <- max(w + gamma d, 0) for entry j, unless the status word says that a factorisation failed (now or earlier)
static __device__ __forceinline__ void qn_apply(const QnArgs& a, int j, double d, bool ok) {
  double x = a.w[j];
  if (ok) {
    x = bcx_clamp0(x + a.sched[a.step] * d);
    a.w[j] = x;
    if (a.dir) a.dir[j] = d;
  }
  if (a.trace) a.trace[(size_t)a.step * a.k + j] = x;
}

// ---- k <= QN_SINGLE_MAX: one workgroup, the lower triangle and the right-hand side (row k) in LDS ---------------------------------
__global__ __launch_bounds__(QN_SMALL_THREADS) void qn_small_kernel(QnArgs a) {
  extern __shared__ double qs[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int k = a.k, ld = k + 1;                    // (odd or even: rows are walked by lanes along columns, columns by one lane per row)
  double* sA = qs;                                  // (k + 1) x ld
  double* sdiag = qs + (size_t)(k + 1) * ld;        // k: the pivots' square roots
  double* sd = sdiag + k;                           // k: the direction
  const int st0 = *a.status;
  const double shift = (double)a.S * a.tau;
  for (int e = tid; e < k * k; e += QN_SMALL_THREADS) {
    const int i = e / k, j = e - i * k;
    if (j <= i) sA[i * ld + j] = a.G[(size_t)i * a.kp + j] + (i == j ? shift : 0.0);
  }
  for (int j = tid; j < k; j += QN_SMALL_THREADS) sA[k * ld + j] = a.y[j];
  __syncthreads();
  bool fail = false;
  for (int c = 0; c < k; ++c) {
    const double piv = sA[c * ld + c];
    if (!(piv > 0.0)) { fail = true; break; }       // (every thread reads the same value: the branch is uniform)
    const double l = sqrt(piv);
    for (int r = c + 1 + tid; r <= k; r += QN_SMALL_THREADS) sA[r * ld + c] /= l;
    if (tid == 0) sdiag[c] = l;
    __syncthreads();
    for (int r = c + 1 + wave; r <= k; r += QN_SMALL_THREADS / 64) {
      const double lrc = sA[r * ld + c];
      const int cend = min(r, k - 1);
      for (int c2 = c + 1 + lane; c2 <= cend; c2 += 64) sA[r * ld + c2] -= lrc * sA[c2 * ld + c];
    }
    __syncthreads();
  }
  if (fail) {
    if (tid == 0) atomicMax(a.status, 1);
  } else {
    for (int c = k - 1; c >= 0; --c) {              // L^T d = y, y in row k
      const double dc = sA[k * ld + c] / sdiag[c];
      if (tid == 0) sd[c] = dc;
      for (int r = tid; r < c; r += QN_SMALL_THREADS) sA[k * ld + r] -= sA[c * ld + r] * dc;
      __syncthreads();
    }
  }
  const bool ok = !fail && st0 == 0;
  for (int j = tid; j < k; j += QN_SMALL_THREADS) qn_apply(a, j, ok ? sd[j] : 0.0, ok);
}

// ---- the blocked form ----------------------------------------------------------------------------------------------------------------
// Entries of the kp x kp matrix with an index >= k are the identity's and exist only in the loads below: the Gram kernel writes
// the k x k part, and no kernel reads or writes a row or column beyond it.
__global__ __launch_bounds__(64) void qn_diag_kernel(QnArgs a, int jj) {
  const int lane = threadIdx.x, l = lane & 31, row = jj + l;
  const bool lower = lane < 32;
  const double shift = (double)a.S * a.tau;
  double t[QN_NB];
#pragma unroll
  for (int c = 0; c < QN_NB; ++c) {
    const int col = jj + c;
    double v = (c == l) ? 1.0 : 0.0;                // (lanes 32 .. 63: the identity; the padding: the identity)
    if (lower && c <= l && row < a.k) v = a.G[(size_t)row * a.kp + col] + (c == l ? shift : 0.0);
    t[c] = v;
  }
  double dmin;
  chol32_factor(t, dmin);
  if (lane == 0 && !(dmin > 0.0)) atomicMax(a.status, 1);      // (NaN included)
  double* Tj = a.T + (size_t)(jj / QN_NB) * QN_NB * QN_NB;
#pragma unroll
  for (int c = 0; c < QN_NB; ++c) {
    if (lower) { if (c <= l && row < a.k) a.G[(size_t)row * a.kp + jj + c] = t[c]; }
    else Tj[c * QN_NB + l] = c >= l ? t[c] : 0.0;   // lane 32 + l holds row l of L^-T: T[c][l] = (L^-1)[c][l]
  }
  // the panel's entries of y = L^-1 (V resid): the rows above have been subtracted by the update launches before this one
  double bl = lower ? a.y[row] : 0.0;
#pragma unroll
  for (int c = 0; c < QN_NB; ++c) {
    if (lane == c) bl = bl / t[c];
    const double yc = lp_readlane(bl, c);
    if (lower && l > c) bl = fma(-t[c], yc, bl);
  }
  if (lower) a.y[row] = bl;
}

// L21 = A21 T^T for 64 rows below the diagonal tile
__global__ __launch_bounds__(256) void qn_panel_kernel(QnArgs a, int jj) {
  __shared__ double sT[QN_NB][QN_NB + 1];
  __shared__ double sR[QN_UB][QN_NB + 1];
  const int tid = threadIdx.x;
  const int r0 = jj + QN_NB + blockIdx.x * QN_UB;
  const double* Tj = a.T + (size_t)(jj / QN_NB) * QN_NB * QN_NB;
  for (int e = tid; e < QN_NB * QN_NB; e += 256) sT[e >> 5][e & 31] = Tj[e];
  for (int e = tid; e < QN_UB * QN_NB; e += 256) {
    const int r = e >> 5, c = e & 31;
    sR[r][c] = r0 + r < a.k ? a.G[(size_t)(r0 + r) * a.kp + jj + c] : 0.0;
  }
  __syncthreads();
  const int r = tid >> 2;                             // thread -> row tid / 4, columns (tid % 4) + 4 u
  if (r0 + r >= a.k) return;
#pragma unroll
  for (int u = 0; u < QN_NB / 4; ++u) {
    const int c = (tid & 3) + 4 * u;
    double acc = 0.0;
    for (int x = 0; x <= c; ++x) acc += sR[r][x] * sT[c][x];
    a.G[(size_t)(r0 + r) * a.kp + jj + c] = acc;
  }
}

// A22[bi][bj] -= L21[bi] L21[bj]^T over the 64 x 64 blocks bi >= bj of the trailing matrix (workgroups 0 .. ntri - 1: each wave a
// 32 x 32 quadrant as 2 x 2 tiles of v_mfma_f64_16x16x4_f64), and y2 -= L21 y1 (workgroups ntri ..: 64 rows each)
__global__ __launch_bounds__(256) void qn_update_kernel(QnArgs a, int jj, int ntri) {
  __shared__ double sI[QN_NB][QN_LDT];               // [x][i] = L21[ri + i][x]
  __shared__ double sJ[QN_NB][QN_LDT];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int base = jj + QN_NB;
  if ((int)blockIdx.x >= ntri) {
    const int row = base + ((int)blockIdx.x - ntri) * QN_UB + tid;
    if (tid < QN_UB && row < a.k) {
      const double* lr = a.G + (size_t)row * a.kp + jj;
      double v[QN_NB];
#pragma unroll
      for (int x = 0; x < QN_NB; ++x) v[x] = lr[x];
      double acc = a.y[row];
#pragma unroll
      for (int x = 0; x < QN_NB; ++x) acc -= v[x] * a.y[jj + x];
      a.y[row] = acc;
    }
    return;
  }
  int t = blockIdx.x, bi = 0;
  while (t > bi) { t -= bi + 1; ++bi; }
  const int bj = t;
  const int ri = base + bi * QN_UB, rj = base + bj * QN_UB;
  for (int e = tid; e < QN_UB * QN_NB; e += 256) {
    const int r = e >> 5, c = e & 31;
    sI[c][r] = ri + r < a.k ? a.G[(size_t)(ri + r) * a.kp + jj + c] : 0.0;
    sJ[c][r] = rj + r < a.k ? a.G[(size_t)(rj + r) * a.kp + jj + c] : 0.0;
  }
  __syncthreads();
  const int li = lane & 15, lk = lane >> 4;
  const int wi = 32 * (wave >> 1), wj = 32 * (wave & 1);
  qn4d acc[2][2];
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int v = 0; v < 2; ++v) acc[u][v] = (qn4d){0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int ks = 0; ks < QN_NB / 4; ++ks) {
    double av[2], bv[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) { av[u] = sI[4 * ks + lk][wi + 16 * u + li]; bv[u] = sJ[4 * ks + lk][wj + 16 * u + li]; }
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int v = 0; v < 2; ++v) acc[u][v] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[u], bv[v], acc[u][v], 0, 0, 0);
  }
  // f64 C/D layout: column = lane & 15, row = (lane >> 4) + 4 * register
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int v = 0; v < 2; ++v)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = ri + wi + 16 * u + lk + 4 * r, col = rj + wj + 16 * v + li;
        if (col <= row && row < a.k) a.G[(size_t)row * a.kp + col] -= acc[u][v][r];
      }
}

// L^T d = y from the last panel to the first, then the update.  One workgroup; y (then d) lives in LDS.
__global__ __launch_bounds__(QN_BACK_THREADS) void qn_back_kernel(QnArgs a) {
  __shared__ double sy[QN_KMAX];
  __shared__ double sdj[QN_NB];
  const int tid = threadIdx.x;
  const int st0 = *a.status;                          // (the diagonal launches of this step have raised it by now)
  for (int i = tid; i < a.kp; i += QN_BACK_THREADS) sy[i] = a.y[i];
  for (int jj = a.kp - QN_NB; jj >= 0; jj -= QN_NB) {
    __syncthreads();
    if (tid < QN_NB) {                                // d_j = T_j^T z: T is lower triangular
      const double* Tj = a.T + (size_t)(jj / QN_NB) * QN_NB * QN_NB;
      double acc = 0.0;
      for (int x = tid; x < QN_NB; ++x) acc += Tj[x * QN_NB + tid] * sy[jj + x];
      sdj[tid] = acc;
    }
    __syncthreads();
    if (tid < QN_NB) sy[jj + tid] = sdj[tid];
    const int nr = min(QN_NB, a.k - jj);              // (rows of the padding are the identity's: nothing left of the diagonal)
    for (int i = tid; i < jj; i += QN_BACK_THREADS) {
      double acc = sy[i];
#pragma unroll 8
      for (int x = 0; x < nr; ++x) acc -= a.G[(size_t)(jj + x) * a.kp + i] * sdj[x];
      sy[i] = acc;
    }
  }
  __syncthreads();
  const bool ok = st0 == 0;
  for (int j = tid; j < a.k; j += QN_BACK_THREADS) qn_apply(a, j, sy[j], ok);
}

// ---- host side -------------------------------------------------------------------------------------------------------------------------
static int64_t qn_even(int64_t n) { return (n + 1) & ~(int64_t)1; }
struct QnLayout { int64_t y, part, Vc, G, T, gram, total; int Sp, kp, nslab; };      // offsets in doubles; total in bytes
static QnLayout qn_layout(int k, int S) {
  QnLayout L;
  L.Sp = (int)qn_even(S);
  L.kp = (k + QN_NB - 1) / QN_NB * QN_NB;
  L.nslab = (k + QN_ROWS - 1) / QN_ROWS;
  const bool blocked = k > QN_SINGLE_MAX;
  int64_t o = 0;
  L.y = o; o += L.kp;
  L.part = o; o += qn_even((int64_t)L.nslab * S);
  L.Vc = o; o += (int64_t)k * L.Sp;
  L.G = o; o += (int64_t)(blocked ? L.kp : k) * L.kp;
  L.T = o; o += blocked ? (int64_t)L.kp * QN_NB : 0;
  L.gram = o;
  L.total = o * (int64_t)sizeof(double) + qn_even((bcx_gram_tiled_scratch_bytes(k, L.Sp) + 7) / 8) * (int64_t)sizeof(double);
  return L;
}

extern "C" int64_t bcx_quasi_newton_scratch_bytes(int32_t k, int32_t S) {
  if (k < 1 || k > QN_KMAX || S < 1 || S > QN_SMAX) return -1;
  return qn_layout(k, S).total;
}

extern "C" int bcx_quasi_newton_step(void* stream, int32_t k, int32_t S, const void* colsum_dev, double scaling, const void* core_dev,
                                     int64_t ldc, int32_t core_is_raw, void* w_dev, const void* sched_dev, int32_t step, double tau,
                                     void* dir_dev, void* trace_dev, void* status_dev, void* work_dev, int64_t work_bytes) {
  if (k < 1 || k > QN_KMAX || S < 1 || S > QN_SMAX || ldc < S || step < 0 || !(tau >= 0.0) || !colsum_dev || !core_dev || !w_dev ||
      !sched_dev || !status_dev || !work_dev || ((uintptr_t)work_dev & 15) || work_bytes < bcx_quasi_newton_scratch_bytes(k, S))
    return bcx_fail(BCX_ERR_ARG, "bcx_quasi_newton_step", "bad arguments (1 <= k <= 4096 weights, 1 <= S <= 8192, ldc >= S, tau >= 0, 16-byte "
                                                          "aligned scratch of bcx_quasi_newton_scratch_bytes(k, S) bytes)");
  const QnLayout L = qn_layout(k, S);
  double* work = (double*)work_dev;
  QnArgs a;
  a.colsum = (const double*)colsum_dev; a.core = (const double*)core_dev; a.sched = (const double*)sched_dev;
  a.w = (double*)w_dev; a.dir = (double*)dir_dev; a.trace = (double*)trace_dev; a.status = (int*)status_dev;
  a.y = work + L.y; a.part = work + L.part; a.Vc = work + L.Vc; a.G = work + L.G; a.T = work + L.T;
  a.scaling = scaling; a.tau = tau; a.ldc = ldc; a.k = k; a.S = S; a.Sp = L.Sp; a.kp = L.kp; a.step = step; a.raw_core = core_is_raw;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(qn_center_kernel, dim3(L.nslab), dim3(256), 0, st, a);
  hipLaunchKernelGGL(qn_rhs_kernel, dim3(L.nslab), dim3(256), (size_t)S * sizeof(double), st, a);
  BCX_TRY("bcx_quasi_newton_step", hipGetLastError());
  const int rc = bcx_gram_rows_tiled(st, a.Vc, k, L.Sp, (int64_t)L.Sp, a.G, (int64_t)L.kp, work + L.gram);
  if (rc != BCX_OK) return rc;                        // (the text names bcx_gram, whose kernel it is)
  if (k <= QN_SINGLE_MAX) {
    const size_t lds = QN_SMALL_LDS(k);
    static PerDevice<size_t> lds_max;
    BCX_TRY("bcx_quasi_newton_step", raise_dynamic_lds((const void*)qn_small_kernel, lds, 32 * 1024, lds_max));
    hipLaunchKernelGGL(qn_small_kernel, dim3(1), dim3(QN_SMALL_THREADS), lds, st, a);
  } else {
    for (int jj = 0; jj < L.kp; jj += QN_NB) {
      hipLaunchKernelGGL(qn_diag_kernel, dim3(1), dim3(64), 0, st, a, jj);
      const int below = k - jj - QN_NB;               // rows under the tile that exist
      if (below > 0) {
        const int nb = (below + QN_UB - 1) / QN_UB, ntri = nb * (nb + 1) / 2;
        hipLaunchKernelGGL(qn_panel_kernel, dim3(nb), dim3(256), 0, st, a, jj);
        hipLaunchKernelGGL(qn_update_kernel, dim3(ntri + nb), dim3(256), 0, st, a, jj, ntri);
      }
    }
    hipLaunchKernelGGL(qn_back_kernel, dim3(1), dim3(QN_BACK_THREADS), 0, st, a);
  }
  BCX_TRY("bcx_quasi_newton_step", hipGetLastError());
  return BCX_OK;
}
