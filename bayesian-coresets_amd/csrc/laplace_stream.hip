// laplace_stream.hip -- the Laplace fit-and-draw of csrc/laplace.hip for points that do not fit one workgroup's LDS (coresets
// beyond k (D + 5) 8 B = 96 KiB, the resident full data set): the same objective, damped Newton iteration, status word and
// output buffers, the k points STREAMED from device memory by G co-resident workgroups in one persistent launch.
//
//  * a workgroup owns a contiguous range of 128-row tiles; per tile it stages the rows in LDS (row stride ldp), evaluates
//    lap_point at the candidates of the current step-halving batch (two threads per row, two candidates each) and adds, in
//    fp64, the objective at every candidate and -- at the batch's first candidate -- sum_j w_j g_j x_j and the lower triangle of
//    sum_j w_j h_j x_j x_j^T (one matrix entry per thread and row slice, kept in registers over the workgroup's tiles);
//  * it writes ONE partial record per pass; after the grid barrier (GridSync / grid_barrier of nnls_common.h, bounded wait)
//    EVERY workgroup adds the G records in workgroup order -- no floating-point atomics, so a fit is bit-reproducible for a
//    given (k, D, G) -- and takes the Newton step itself: all workgroups hold the same iterate bit for bit, decide alike and
//    leave together.  One barrier per pass; a solving workgroup that publishes would need a second one per pass to hand the
//    step back, and the solve (a 32 x 32 Cholesky in one wave, ~10 us) is idle time for the others either way;
//  * the step-halving ladder goes in batches of four (t, t/2, t/4, t/8; derivatives at t): an iteration whose full step is
//    accepted costs one pass over the rows, one that halves costs two (the second one for the derivatives where it landed).
// The records of pass p live in half p & 1 of the work buffer: a workgroup writes half p & 1 again only after barrier p + 1,
// which every reader of pass p has reached -- no workgroup is ever more than one barrier ahead of another (the invariant the
// barrier of nnls_common.h rests on).
#include <algorithm>
#include <string>
#include "bcx_internal.h"
#include "dev_util.h"
#include "nnls_common.h"
#include "chol32.h"
#include "lik_point.h"
#include "launch_host.h"

#define LS_DMAX 32
#define LS_THREADS 256
#define LS_TILE 128
#define LS_BATCH 4
#define LS_MAX_WGS 256          // one record per workgroup is read by every workgroup after every pass
#define LS_SYNC_BYTES 128       // the arrival counter, alone in the first 128 bytes of the work buffer (zeroed before every launch)

struct LapStreamArgs {
  const double* w;
  const double* pts;
  double* mu;
  const double* R;
  const double* Rbar;
  double* theta;
  double* tbar;
  int* status;          // as laplace_sampler_kernel's, plus [0] = 3: a grid barrier timed out
  double* part;         // 2 x G x rec doubles
  double tol;
  int64_t ldp;
  int family, k, D, S, ld, max_iter, warm, rec;
};

static __host__ __device__ inline int ls_entries(int D) { return D + D * (D + 1) / 2; }
static __host__ __device__ inline int ls_record(int D) { return LS_BATCH + ls_entries(D); }

__global__ __launch_bounds__(LS_THREADS) void laplace_stream_kernel(LapStreamArgs a, GridSync gs) {
  __shared__ double sX[LS_TILE * 33];
  __shared__ double s_dg[32 * 33], s_W[32 * 33];
  __shared__ double s_tot[LS_BATCH + LS_DMAX + LS_DMAX * (LS_DMAX + 1) / 2];
  __shared__ double s_red[LS_THREADS];
  __shared__ double s_coef[2 * LS_TILE];             // w_j g_j, then w_j h_j of the tile's rows
  __shared__ double s_w[LS_TILE], s_yv[LS_TILE];
  __shared__ double s_cand[LS_BATCH][32];
  __shared__ double s_th[32], s_grad[32], s_step[32], s_y[32];
  __shared__ double scratch[BCX_SCRATCH];
  __shared__ int s_bad, s_flag;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wg = blockIdx.x, G = gridDim.x;
  const int k = a.k, D = a.D;
  const int Ds = (D + 1) | 1;                         // LDS row: D features, a column of ones, odd stride (rows on different banks)
  const int cols = D + (a.family == LAP_POISSON ? 1 : 0);
  const int E = ls_entries(D);
  const int64_t T = ((int64_t)k + LS_TILE - 1) / LS_TILE;
  const int64_t tile0 = T * wg / G, tile1 = T * (wg + 1) / G;
  // this thread's entries of [sum w g x | lower triangle of sum w h x x^T] and its slice of a tile's rows
  const int Es = E < LS_THREADS ? E : LS_THREADS;
  const int nslice = LS_THREADS / Es;                 // >= 1; E > 256: one slice, up to three entries per thread
  const int slice = tid / Es;
  const bool worker = slice < nslice;
  const int rows_per = (LS_TILE + nslice - 1) / nslice;
  int e_cf[3], e_r[3], e_c[3];
  bool e_on[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const int e = tid % Es + i * LS_THREADS;
    e_on[i] = worker && e < E && (i == 0 || E > LS_THREADS);
    e_cf[i] = 0; e_r[i] = 0; e_c[i] = D;
    if (e_on[i] && e < D) { e_r[i] = e; }             // gradient entry: w g x_e * 1
    else if (e_on[i]) {
      const int p = e - D;
      int r = 0;
      while ((r + 1) * (r + 2) / 2 <= p) ++r;
      e_cf[i] = LS_TILE; e_r[i] = r; e_c[i] = p - r * (r + 1) / 2;
    }
  }
  if (tid < 32) s_th[tid] = (tid < D && a.warm) ? a.mu[tid] : 0.0;
  __syncthreads();

  int bi = 0;                                         // grid barriers passed
  // One pass over the rows: objective sums at s_cand[0 .. nc), derivative sums at s_cand[0]; the totals over all workgroups
  // in s_tot.  false: the barrier timed out.
  auto pass = [&](int nc) -> bool {
    double acc0 = 0.0, acc1 = 0.0, acc2 = 0.0, va = 0.0, vb = 0.0;
    const int sub = tid & 1, rj = tid >> 1;
    const int ca = 2 * sub, cb = 2 * sub + 1;
    for (int64_t tile = tile0; tile < tile1; ++tile) {
      const int64_t row0 = tile * LS_TILE;
      const int rows = (int)((int64_t)k - row0 < LS_TILE ? (int64_t)k - row0 : LS_TILE);
      for (int e = tid; e < LS_TILE * cols; e += LS_THREADS) {
        const int j = e / cols, c = e - j * cols;
        const double v = j < rows ? a.pts[(size_t)(row0 + j) * a.ldp + c] : 0.0;
        if (c < D) sX[j * Ds + c] = v; else s_yv[j] = v;
      }
      if (tid < LS_TILE) {
        s_w[tid] = tid < rows ? bcx_clamp0(a.w[row0 + tid]) : 0.0;
        sX[tid * Ds + D] = 1.0;
        if (a.family != LAP_POISSON) s_yv[tid] = 0.0;
      }
      __syncthreads();
      if (ca < nc) {
        double sa = 0.0, sb = 0.0;
        for (int c = 0; c < D; ++c) {
          const double x = sX[rj * Ds + c];
          sa = fma(x, s_cand[ca][c], sa);
          sb = fma(x, s_cand[cb][c], sb);
        }
        const double wj = s_w[rj], yj = s_yv[rj];
        double ll, g, h;
        lap_point(a.family, sa, yj, ll, g, h);
        va += wj * ll;
        if (sub == 0) { s_coef[rj] = wj * g; s_coef[LS_TILE + rj] = wj * h; }
        if (cb < nc) {
          lap_point(a.family, sb, yj, ll, g, h);
          vb += wj * ll;
        }
      }
      __syncthreads();
      if (worker) {
        const int j0 = slice * rows_per, j1 = j0 + rows_per < LS_TILE ? j0 + rows_per : LS_TILE;
        for (int j = j0; j < j1; ++j) {
          const double* xr = sX + j * Ds;
          acc0 = fma(s_coef[e_cf[0] + j] * xr[e_r[0]], xr[e_c[0]], acc0);
          if (E > LS_THREADS) {
            acc1 = fma(s_coef[e_cf[1] + j] * xr[e_r[1]], xr[e_c[1]], acc1);
            acc2 = fma(s_coef[e_cf[2] + j] * xr[e_r[2]], xr[e_c[2]], acc2);
          }
        }
      }
      __syncthreads();
    }
    // the workgroup's record: objective sums, then the entries (row slices added in slice order)
    double v[LS_BATCH] = {sub ? 0.0 : va, sub ? 0.0 : vb, sub ? va : 0.0, sub ? vb : 0.0};
    block_allsum<LS_BATCH>(v, scratch);
    double* mine = a.part + ((size_t)(bi & 1) * G + wg) * a.rec;
    if (tid < LS_BATCH) coh_store(mine + tid, v[tid]);
    if (E > LS_THREADS) {
      if (e_on[0]) coh_store(mine + LS_BATCH + tid, acc0);
      if (e_on[1]) coh_store(mine + LS_BATCH + tid + LS_THREADS, acc1);
      if (e_on[2]) coh_store(mine + LS_BATCH + tid + 2 * LS_THREADS, acc2);
    } else {
      s_red[tid] = acc0;
      __syncthreads();
      if (tid < E) {
        double t = s_red[tid];
        for (int q = 1; q < nslice; ++q) t += s_red[q * Es + tid];
        coh_store(mine + LS_BATCH + tid, t);
      }
    }
    ++bi;
    if (!grid_barrier(gs, bi, &s_flag)) return false;
    const double* all = a.part + (size_t)((bi - 1) & 1) * G * a.rec;
    for (int i = tid; i < a.rec; i += LS_THREADS) {
      double t = 0.0;
      int g = 0;
      for (; g + 8 <= G; g += 8) {
        double m[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) m[u] = coh_load(all + (size_t)(g + u) * a.rec + i);
#pragma unroll
        for (int u = 0; u < 8; ++u) t += m[u];
      }
      for (; g < G; ++g) t += coh_load(all + (size_t)g * a.rec + i);
      s_tot[i] = t;
    }
    __syncthreads();
    return true;
  };
  // objective at candidate i from the totals
  auto value = [&](int i) -> double {
    double q = 0.0;
    for (int c = 0; c < D; ++c) q = fma(s_cand[i][c], s_cand[i][c], q);
    return s_tot[i] - 0.5 * q;
  };
  // gradient and Newton matrix I - sum_j w_j h_j x_j x_j^T at s_th from the totals, the matrix padded to 32 x 32 with the identity
  auto assemble = [&]() {
    for (int e = tid; e < 32 * 32 + 32; e += LS_THREADS) {
      if (e < 32 * 32) {
        const int r = e >> 5, c = e & 31;
        double v = r == c ? 1.0 : 0.0;
        if (r < D && c < D) { const int hi = r > c ? r : c, lo = r > c ? c : r; v -= s_tot[LS_BATCH + D + hi * (hi + 1) / 2 + lo]; }
        s_dg[r * 33 + c] = v;
      } else {
        const int c = e - 32 * 32;
        s_grad[c] = c < D ? s_tot[LS_BATCH + c] - s_th[c] : 0.0;
      }
    }
    __syncthreads();
  };
  // W = L^-1 of the Newton matrix in s_dg (row-major in s_W); a matrix that is not positive definite gets lambda I added.  The
  // text of laplace.hip's, restated: moved into a shared function it changes that kernel's register allocation (12 B of scratch)
  auto factor = [&]() -> bool {
    double lambda = 0.0;
    for (int attempt = 0; attempt < 24; ++attempt) {
      if (tid == 0) s_bad = 0;
      __syncthreads();
      if (wave == 0) {
        double r[32];
        const int row = lane & 31;
        const bool top = lane < 32;
#pragma unroll
        for (int c = 0; c < 32; ++c) r[c] = top ? (c <= row ? s_dg[row * 33 + c] + (c == row ? lambda : 0.0) : 0.0) : (c == row ? 1.0 : 0.0);
        double dmin;
        chol32_factor(r, dmin);
        if (!(dmin > 0.0)) { if (lane == 0) s_bad = 1; }
        else if (!top) {
#pragma unroll
          for (int c = 0; c < 32; ++c) s_W[c * 33 + row] = r[c];
        }
      }
      __syncthreads();
      if (!s_bad) return true;
      double dmax = 1.0;
      for (int c = 0; c < D; ++c) dmax = fmax(dmax, fabs(s_dg[c * 33 + c]));
      lambda = lambda == 0.0 ? 1e-8 * dmax : lambda * 10.0;
      __syncthreads();
    }
    return false;
  };

  // The iteration of laplace_sampler_kernel as a sequence of passes (ONE call site of pass / assemble / factor: the kernel's
  // text stays small).  A pass is the start (PH_START), a batch of the ladder (PH_BATCH) or the derivatives where a halved
  // step landed (PH_DERIV); after each, s_tot either sends the ladder on or holds the derivative sums at s_th.
  enum { PH_START, PH_BATCH, PH_DERIV };
  int status = 1, steps = 0, it = 0, phase = PH_START, nc = 1;
  bool alive = true, have_W = false;
  double f = 0.0, t = 1.0, smax = 0.0;
  if (tid < 32) s_cand[0][tid] = s_th[tid];
  __syncthreads();
  for (;;) {
    alive = pass(nc);
    if (!alive) break;
    if (phase == PH_START) f = value(0);
    if (phase == PH_BATCH) {                          // damped: the objective must not decrease; t, t / 2, ... in batches of four
      int took = -1;
      double fc = 0.0, ti = t;
      for (int i = 0; i < LS_BATCH; ++i, ti *= 0.5) {
        fc = value(i);
        if (fc >= f || ti < 1e-10) { took = i; t = ti; break; }
      }
      __syncthreads();
      if (took < 0) {
        t *= 1.0 / 16.0;
        if (tid < 32) {
          double tj = t;
          for (int i = 0; i < LS_BATCH; ++i, tj *= 0.5) s_cand[i][tid] = s_th[tid] + tj * s_step[tid];
        }
        __syncthreads();
        continue;
      }
      if (tid < 32) s_th[tid] = s_cand[took][tid];
      f = fc;
      ++steps;
      __syncthreads();
      if (took != 0) {                                // the derivatives where the ladder stopped
        if (tid < 32) s_cand[0][tid] = s_th[tid];
        __syncthreads();
        nc = 1; phase = PH_DERIV;
        continue;
      }
    }
    // s_tot holds the derivative sums at s_th: the next Newton step, or the covariance factor at the mode
    bool last = false;
    if (phase != PH_START && smax * t < a.tol) { status = 0; last = true; }
    else if (it >= a.max_iter) last = true;
    assemble();
    have_W = factor();
    if (!have_W) { status = 2; break; }
    if (last) break;
    ++it;
    if (tid < 32) {                                   // step = W^T (W grad)
      double u = 0.0;
      for (int c = 0; c <= tid; ++c) u = fma(s_W[tid * 33 + c], s_grad[c], u);
      s_y[tid] = u;
    }
    __syncthreads();
    if (tid < 32) {
      double u = 0.0;
      for (int c = tid; c < 32; ++c) u = fma(s_W[c * 33 + tid], s_y[c], u);
      s_step[tid] = tid < D ? u : 0.0;
    }
    __syncthreads();
    smax = 0.0;
    for (int c = 0; c < D; ++c) smax = fmax(smax, fabs(s_step[c]));
    t = 1.0;
    if (tid < 32) {
      double tj = t;
      for (int i = 0; i < LS_BATCH; ++i, tj *= 0.5) s_cand[i][tid] = s_th[tid] + tj * s_step[tid];
    }
    __syncthreads();
    nc = LS_BATCH; phase = PH_BATCH;
  }
  if (!alive) {                                       // a barrier timed out: every workgroup ends here, after its own bounded wait
    if (tid == 0) { atomicMax(&a.status[2], 3); a.status[0] = 3; }
    return;
  }
  if (wg == 0) {
    if (tid < D) a.mu[tid] = s_th[tid];
    if (tid == 0) { a.status[0] = status; a.status[1] = steps; atomicMax(&a.status[2], status); }
  }
  if (!have_W) {                                      // (no factor: the draws are the mode -- the caller raises on the status)
    __syncthreads();
    for (int e = tid; e < 32 * 33; e += LS_THREADS) s_W[e] = 0.0;
    __syncthreads();
  }
  // theta = mu + [R; Rbar] W, the S + 1 rows spread over all workgroups
  const int64_t total = (int64_t)(a.S + 1) * a.ld;
  for (int64_t e = (int64_t)wg * LS_THREADS + tid; e < total; e += (int64_t)G * LS_THREADS) {
    const int s = (int)(e / a.ld), c = (int)(e - (int64_t)s * a.ld);
    double v = 0.0;
    if (c < D) {
      const double* rr = s < a.S ? a.R + (size_t)s * a.ld : a.Rbar;
      v = s_th[c];
      for (int i = c; i < D; ++i) v = fma(rr[i], s_W[i * 33 + c], v);
    }
    if (s < a.S) a.theta[(size_t)s * a.ld + c] = v;
    else if (c < D) a.tbar[c] = v;
  }
}

static int ls_cap_wgs(int64_t k) {
  const int64_t tiles = (k + LS_TILE - 1) / LS_TILE;
  return (int)(tiles < 1 ? 1 : tiles > LS_MAX_WGS ? LS_MAX_WGS : tiles);
}

extern "C" int64_t bcx_laplace_stream_scratch_bytes(int32_t k, int32_t D) {
  if (k < 0 || D < 1 || D > LS_DMAX) return -1;
  return LS_SYNC_BYTES + 2 * (int64_t)ls_cap_wgs(k) * ls_record(D) * (int64_t)sizeof(double);
}

extern "C" int bcx_laplace_sampler_stream(void* stream, int32_t family, int32_t k, int32_t D, const void* w_dev, const void* pts_dev,
                                          int64_t ldp, void* mu_dev, int32_t warm, double tol, int32_t max_iter, const void* R_dev,
                                          const void* Rbar_dev, int32_t S, int32_t ld, void* theta_dev, void* tbar_dev, void* status_dev,
                                          void* work_dev, int64_t work_bytes) {
  if ((family != LAP_LOGISTIC && family != LAP_POISSON) || k < 0 || D < 1 || D > LS_DMAX || S < 1 || ld < D || max_iter < 1 || !(tol > 0.0) ||
      !mu_dev || !R_dev || !Rbar_dev || !theta_dev || !tbar_dev || !status_dev || !work_dev ||
      work_bytes < bcx_laplace_stream_scratch_bytes(k, D) || (k > 0 && (!w_dev || !pts_dev || ldp < D + (family == LAP_POISSON ? 1 : 0))))
    return bcx_fail(BCX_ERR_ARG, "bcx_laplace_sampler_stream", "bad arguments (family 0 logistic / 1 Poisson, D <= 32 parameters, work_dev of "
                                                               "bcx_laplace_stream_scratch_bytes)");
  static PerDevice<int> resident_of;
  const int resident = one_wg_per_cu((const void*)laplace_stream_kernel, LS_THREADS, resident_of);
  if (resident < 1)
    return bcx_fail(BCX_ERR_STATE, "bcx_laplace_sampler_stream", "the kernel's workgroups cannot be resident together on this device");
  const int G = std::min(ls_cap_wgs(k), resident);
  LapStreamArgs a;
  a.w = (const double*)w_dev; a.pts = (const double*)pts_dev; a.mu = (double*)mu_dev; a.R = (const double*)R_dev;
  a.Rbar = (const double*)Rbar_dev; a.theta = (double*)theta_dev; a.tbar = (double*)tbar_dev; a.status = (int*)status_dev;
  a.part = (double*)((char*)work_dev + LS_SYNC_BYTES);
  a.tol = tol; a.ldp = ldp; a.family = family; a.k = k; a.D = D; a.S = S; a.ld = ld; a.max_iter = max_iter; a.warm = warm;
  a.rec = ls_record(D);
  const GridSync gs = grid_sync_at((unsigned long long*)work_dev, 200000000LL);         // 2 s of the 100 MHz wall clock per wait
  BCX_TRY("bcx_laplace_sampler_stream", hipMemsetAsync(work_dev, 0, LS_SYNC_BYTES, (hipStream_t)stream));
  hipLaunchKernelGGL(laplace_stream_kernel, dim3(G), dim3(LS_THREADS), 0, (hipStream_t)stream, a, gs);
  BCX_TRY("bcx_laplace_sampler_stream", hipGetLastError());
  return BCX_OK;
}
