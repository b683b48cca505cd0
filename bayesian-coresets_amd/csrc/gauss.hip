// gauss.hip -- the pieces of the Gaussian-mean family (reference: examples/common/model_gaussian.py, examples/gaussian/main.py)
// that are not the projection itself (csrc/proj.hip FAM_GAUSSIAN) or the pseudo-point gradient (csrc/psvi.hip PS_GAUSSIAN):
//
//   gauss_mean_kernel      tbar = the mean of the draws, as theta_0 + mean_s (theta_s - theta_0): equal draws give tbar = theta_0 to the bit
//   gauss_operand_kernel   rows X (draws or points)  ->  Siginv (x - tbar), with one more value behind every row:
//                            draws : bias_s = -(tbar + (theta_s - tbar) / 2) . g_s     (the projection's Theta operand, proj.hip loglik_col)
//                            points: the mean of the row's D coordinates             (projector.py:26 centres gradients over them)
//   gauss_xsum_*           sum_n x_n of a data set, in one fixed order (slabs of rows per workgroup, partials added in slab order)
//   gauss_colsum_kernel    the column sums of the projected data in closed form: sum_n vecs[n, s] = (sum_n x_n) . g_s + N bias_s, centred over s
//   gps_prep / gps_draw    draws of the weighted posterior (model_gaussian.py:23-30).  Its precision Sig0inv + (sum w) Siginv depends on
//                          the weights only through their sum: with Siginv = L L', L^-1 Sig0inv L^-T = V diag(lam) V' (host, once) and
//                          W = L^-T V the covariance is W diag(1 / (lam + sum w)) W', so a call is two reductions over the points
//                          (sum w, sum_i w_i p_i), three D x D products with a vector for the mean, and theta = mu_w + (R scale) W'
//                          with scale = (lam + sum w)^-1/2 -- no factorisation.  Row S of the product is the same map of the column means
//                          of R: the mean of the draws, which the projection expands around.
// Every sum has one fixed order and there are no atomics.  All entries are asynchronous on `stream`; errors: bcx_project_last_error().
#include <string>
#include "bcx_internal.h"
#include "dev_util.h"
#include "launch_host.h"



#define GS_MAX_DIM 4096       // coordinates (the operand kernel keeps one row in LDS)

// tbar[j] = theta[0][j] + (1 / n) sum_s (theta[s][j] - theta[0][j]), a thread per coordinate, s ascending
__global__ __launch_bounds__(256) void gauss_mean_kernel(const double* __restrict__ theta, int n, int64_t ldt, int D, double* __restrict__ tbar) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= D) return;
  const double t0 = theta[j];
  double acc = 0.0;
  for (int s = 1; s < n; ++s) acc += theta[(int64_t)s * ldt + j] - t0;
  tbar[j] = t0 + acc / (double)n;
}

// One workgroup per row.  Siginv is symmetric: coordinate j of Siginv d is read down column j (adjacent threads, adjacent addresses).
template <bool BIAS>
__global__ __launch_bounds__(256) void gauss_operand_kernel(const double* __restrict__ X, int64_t ldx, int D, const double* __restrict__ Sig,
                                                            int64_t lds, const double* __restrict__ tbar, double* __restrict__ out, int64_t ldo) {
  extern __shared__ __attribute__((aligned(16))) double gs_d[];        // D: x - tbar
  __shared__ double scratch[BCX_SCRATCH];
  const int64_t row = blockIdx.x;
  const double* x = X + row * ldx;
  for (int j = threadIdx.x; j < D; j += 256) gs_d[j] = x[j] - tbar[j];
  __syncthreads();
  double part[1] = {0.0};
  for (int j = threadIdx.x; j < D; j += 256) {
    double g = gs_d[j];
    if (Sig) {
      g = 0.0;
      for (int i = 0; i < D; ++i) g = fma(Sig[(int64_t)i * lds + j], gs_d[i], g);
    }
    out[row * ldo + j] = g;
    part[0] += BIAS ? -(fma(0.5, gs_d[j], tbar[j]) * g) : g;
  }
  block_allsum<1>(part, scratch);
  if (threadIdx.x == 0) out[row * ldo + D] = BIAS ? part[0] : part[0] / (double)D;
}

extern "C" int bcx_gaussian_operand(void* stream, const void* rows_dev, int32_t n, int64_t ldx, int32_t D, const void* Siginv_dev,
                                    int64_t ldsig, const void* tbar_dev, void* out_dev, int64_t ldo, int32_t mode, void* work_dev) {
  static const char* who = "bcx_gaussian_operand";
  if (!rows_dev || !out_dev || n < 0 || D < 1 || D > GS_MAX_DIM || ldx < D || ldo < D + 1) return bcx_fail(BCX_ERR_ARG, who, "bad arguments (1 <= D <= 4096, ldo >= D + 1)");
  if (Siginv_dev && ldsig < D) return bcx_fail(BCX_ERR_ARG, who, "Siginv leading dimension shorter than D");
  if (mode != 0 && mode != 1) return bcx_fail(BCX_ERR_ARG, who, "mode must be 0 (draws: bias) or 1 (points: coordinate mean)");
  if (!tbar_dev && !work_dev) return bcx_fail(BCX_ERR_ARG, who, "without tbar_dev the mean of the rows is formed in work_dev (D doubles)");
  if (n == 0) return BCX_OK;
  hipStream_t st = (hipStream_t)stream;
  const double* tbar = (const double*)tbar_dev;
  if (!tbar) {
    hipLaunchKernelGGL(gauss_mean_kernel, dim3((D + 255) / 256), dim3(256), 0, st, (const double*)rows_dev, (int)n, ldx, (int)D, (double*)work_dev);
    tbar = (const double*)work_dev;
  }
  const size_t lds = (size_t)D * sizeof(double);
  if (mode == 0)
    hipLaunchKernelGGL(gauss_operand_kernel<true>, dim3(n), dim3(256), lds, st, (const double*)rows_dev, ldx, (int)D, (const double*)Siginv_dev,
                       ldsig, tbar, (double*)out_dev, ldo);
  else
    hipLaunchKernelGGL(gauss_operand_kernel<false>, dim3(n), dim3(256), lds, st, (const double*)rows_dev, ldx, (int)D, (const double*)Siginv_dev,
                       ldsig, tbar, (double*)out_dev, ldo);
  BCX_TRY(who, hipGetLastError());
  return BCX_OK;
}

// ---- first moment of a data set -------------------------------------------------------------------------------------------------
// Workgroup b sums rows [b R, (b + 1) R): thread (c = tid % 64, q = tid / 64) the rows q, q + 4, ... of columns c, c + 64, ...; the four
// row classes are added 0..3.  part: gridDim.x x D.
#define GS_XSUM_MAX_SLABS 1024
__global__ __launch_bounds__(256) void gauss_xsum_part_kernel(const double* __restrict__ Z, int64_t N, int64_t ldz, int D, int64_t R,
                                                              double* __restrict__ part) {
  __shared__ double seg[4][64];
  const int c0 = threadIdx.x & 63, q = threadIdx.x >> 6;
  const int64_t lo = (int64_t)blockIdx.x * R, hi = lo + R < N ? lo + R : N;
  for (int cb = 0; cb < D; cb += 64) {
    const int c = cb + c0;
    double acc = 0.0;
    if (c < D)
      for (int64_t n = lo + q; n < hi; n += 4) acc += Z[n * ldz + c];
    seg[q][c0] = acc;
    __syncthreads();
    if (q == 0 && c < D) part[(int64_t)blockIdx.x * D + c] = ((seg[0][c0] + seg[1][c0]) + seg[2][c0]) + seg[3][c0];
    __syncthreads();
  }
}
__global__ __launch_bounds__(256) void gauss_xsum_reduce_kernel(const double* __restrict__ part, int nparts, int D, double* __restrict__ xsum) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= D) return;
  double acc = 0.0;
  for (int b = 0; b < nparts; ++b) acc += part[(int64_t)b * D + c];
  xsum[c] = acc;
}
static int64_t gs_slab_rows(int64_t N) {
  const int64_t r = (N + GS_XSUM_MAX_SLABS - 1) / GS_XSUM_MAX_SLABS;
  return r < 64 ? 64 : r;
}
extern "C" int64_t bcx_gaussian_first_moment_scratch_bytes(int64_t N, int32_t D) {
  if (N < 0 || D < 1) return -1;
  const int64_t R = gs_slab_rows(N), slabs = N ? (N + R - 1) / R : 1;
  return slabs * D * (int64_t)sizeof(double);
}
extern "C" int bcx_gaussian_first_moment(void* stream, const void* Z_dev, int64_t N, int64_t ldz, int32_t D, void* xsum_dev, void* work_dev,
                                         int64_t work_bytes) {
  static const char* who = "bcx_gaussian_first_moment";
  if (!Z_dev || !xsum_dev || !work_dev || N < 0 || D < 1 || ldz < D) return bcx_fail(BCX_ERR_ARG, who, "bad arguments");
  if (work_bytes < bcx_gaussian_first_moment_scratch_bytes(N, D)) return bcx_fail(BCX_ERR_ARG, who, "scratch too small");
  hipStream_t st = (hipStream_t)stream;
  const int64_t R = gs_slab_rows(N);
  const int slabs = (int)(N ? (N + R - 1) / R : 0);
  if (slabs)
    hipLaunchKernelGGL(gauss_xsum_part_kernel, dim3(slabs), dim3(256), 0, st, (const double*)Z_dev, N, ldz, (int)D, R, (double*)work_dev);
  hipLaunchKernelGGL(gauss_xsum_reduce_kernel, dim3((D + 255) / 256), dim3(256), 0, st, (const double*)work_dev, slabs, (int)D, (double*)xsum_dev);
  BCX_TRY(who, hipGetLastError());
  return BCX_OK;
}

// raw[s] = xsum . g_s + n_rows bias_s: a wave per column (lane-strided partial sums, then the wave butterfly)
__global__ __launch_bounds__(256) void gauss_colsum_kernel(const double* __restrict__ xsum, double n_rows, int D, const double* __restrict__ op,
                                                           int S, int64_t ldt, double* __restrict__ colsum) {
  const int lane = threadIdx.x & 63, s = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (s >= S) return;                                   // (wave-uniform)
  const double* g = op + (int64_t)s * ldt;
  double acc = 0.0;
  for (int j = lane; j < D; j += 64) acc = fma(xsum[j], g[j], acc);
  acc = wave_allsum(acc);
  if (lane == 0) colsum[s] = fma(n_rows, g[D], acc);
}
// colsum -= mean(colsum)   (the centring of projector.py:21, summed over the rows)
__global__ __launch_bounds__(256) void gauss_center_kernel(int S, double* __restrict__ colsum) {
  __shared__ double scratch[BCX_SCRATCH];
  double tot[1] = {0.0};
  for (int c = threadIdx.x; c < S; c += 256) tot[0] += colsum[c];
  block_allsum<1>(tot, scratch);
  const double corr = tot[0] / (double)S;
  for (int c = threadIdx.x; c < S; c += 256) colsum[c] -= corr;
}
extern "C" int bcx_gaussian_colsum_moments(void* stream, const void* xsum_dev, double n_rows, int32_t D, const void* operand_dev, int32_t S,
                                           int64_t ldt, void* colsum_dev) {
  static const char* who = "bcx_gaussian_colsum_moments";
  if (!xsum_dev || !operand_dev || !colsum_dev || D < 1 || S < 1 || ldt < D + 1) return bcx_fail(BCX_ERR_ARG, who, "bad arguments (ldt >= D + 1)");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(gauss_colsum_kernel, dim3((S + 3) / 4), dim3(256), 0, st, (const double*)xsum_dev, n_rows, (int)D, (const double*)operand_dev,
                     (int)S, ldt, (double*)colsum_dev);
  hipLaunchKernelGGL(gauss_center_kernel, dim3(1), dim3(256), 0, st, (int)S, (double*)colsum_dev);
  BCX_TRY(who, hipGetLastError());
  return BCX_OK;
}

// ---- the weighted posterior's sampler ----------------------------------------------------------------------------------------------
#define GPS_MAX_DIM 1024
struct GpsArgs {
  int k, D, S, ld;
  const double* w;       // k weights (device)
  const double* pts;     // k x ldp
  int64_t ldp;
  const double* c0;      // Sig0inv mu0
  const double* Sig;     // Siginv (D x D, symmetric) or nullptr: identity
  const double* W;       // D x D, row-major: W = L^-T V
  const double* WT;      // its transpose
  const double* lam;     // D
  const double* R;       // S x ld normal numbers
  const double* Rbar;    // ld: their column means
  double* theta;         // S x ld
  double* tbar;          // D
  double* state;         // [mu (D) | scale (D)]
  int* status;           // |= 1: a precision lam + sum w that is not positive (NaN weights included)
};

// one workgroup: sum w, sum_i w_i p_i (i ascending), u = c0 + Siginv sp, v = (W' u) / prec, mu = W v, scale = prec^-1/2
__global__ __launch_bounds__(256) void gps_prep_kernel(GpsArgs a) {
  __shared__ double va[GPS_MAX_DIM], vb[GPS_MAX_DIM];
  __shared__ int bad;
  const int D = a.D, tid = threadIdx.x;
  if (tid == 0) bad = 0;
  double sw = 0.0;
  for (int i = 0; i < a.k; ++i) sw += a.w[i];
  for (int j = tid; j < D; j += 256) {
    double acc = 0.0;
    for (int i = 0; i < a.k; ++i) acc = fma(a.w[i], a.pts[(int64_t)i * a.ldp + j], acc);
    va[j] = acc;                                        // sp
  }
  __syncthreads();
  for (int j = tid; j < D; j += 256) {
    double acc = va[j];
    if (a.Sig) {
      acc = 0.0;
      for (int i = 0; i < D; ++i) acc = fma(a.Sig[(int64_t)i * D + j], va[i], acc);
    }
    vb[j] = a.c0[j] + acc;                              // u
  }
  __syncthreads();
  for (int m = tid; m < D; m += 256) {
    double acc = 0.0;
    for (int j = 0; j < D; ++j) acc = fma(a.W[(int64_t)j * D + m], vb[j], acc);
    const double prec = a.lam[m] + sw;
    if (!(prec > 0.0)) bad = 1;
    va[m] = acc / prec;                                 // v
    a.state[D + m] = 1.0 / sqrt(prec);
  }
  __syncthreads();
  for (int j = tid; j < D; j += 256) {
    double acc = 0.0;
    for (int m = 0; m < D; ++m) acc = fma(a.WT[(int64_t)m * D + j], va[m], acc);
    a.state[j] = acc;                                   // mu_w
  }
  if (tid == 0 && bad) a.status[0] = 1;
}

// theta[s][j] = mu_j + sum_m WT[m][j] (R[s][m] scale_m); a workgroup takes 16 rows x 64 coordinates, m in runs of 64 through LDS.
// Row S is the image of the column means: tbar.
__global__ __launch_bounds__(256) void gps_draw_kernel(GpsArgs a) {
  __shared__ double rt[16][65];
  const int D = a.D, S = a.S, jx = threadIdx.x & 63, ry = threadIdx.x >> 6;
  const int j = blockIdx.x * 64 + jx, s0 = blockIdx.y * 16;
  const double* scale = a.state + D;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  for (int mb = 0; mb < D; mb += 64) {
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int r = ry + 4 * q, s = s0 + r, m = mb + jx;
      double v = 0.0;
      if (m < D && s <= S) v = (s < S ? a.R[(int64_t)s * a.ld + m] : a.Rbar[m]) * scale[m];
      rt[r][jx] = v;
    }
    __syncthreads();
    if (j < D) {
      const int mend = D - mb < 64 ? D - mb : 64;
      for (int mm = 0; mm < mend; ++mm) {
        const double wv = a.WT[(int64_t)(mb + mm) * D + j];
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[q] = fma(wv, rt[ry + 4 * q][mm], acc[q]);
      }
    }
  }
  if (j < D) {
    const double mu = a.state[j];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int s = s0 + ry + 4 * q;
      if (s < S) a.theta[(int64_t)s * a.ld + j] = mu + acc[q];
      else if (s == S) a.tbar[j] = mu + acc[q];
    }
  }
}

extern "C" int bcx_gaussian_posterior_draw(void* stream, int32_t k, int32_t D, const void* w_dev, const void* pts_dev, int64_t ldp,
                                           const void* c0_dev, const void* Siginv_dev, const void* W_dev, const void* WT_dev,
                                           const void* lam_dev, const void* R_dev, const void* Rbar_dev, int32_t S, int32_t ld,
                                           void* theta_dev, void* tbar_dev, void* state_dev, void* status_dev) {
  static const char* who = "bcx_gaussian_posterior_draw";
  if (k < 0 || D < 1 || D > GPS_MAX_DIM || S < 1 || ld < D) return bcx_fail(BCX_ERR_ARG, who, "bad sizes (1 <= D <= 1024, ld >= D)");
  if (k > 0 && (!w_dev || !pts_dev || ldp < D)) return bcx_fail(BCX_ERR_ARG, who, "weights and points required for k > 0 (ldp >= D)");
  if (!c0_dev || !W_dev || !WT_dev || !lam_dev || !R_dev || !Rbar_dev || !theta_dev || !tbar_dev || !state_dev || !status_dev)
    return bcx_fail(BCX_ERR_ARG, who, "null pointer");
  GpsArgs a;
  a.k = k; a.D = D; a.S = S; a.ld = ld; a.w = (const double*)w_dev; a.pts = (const double*)pts_dev; a.ldp = ldp;
  a.c0 = (const double*)c0_dev; a.Sig = (const double*)Siginv_dev; a.W = (const double*)W_dev; a.WT = (const double*)WT_dev;
  a.lam = (const double*)lam_dev; a.R = (const double*)R_dev; a.Rbar = (const double*)Rbar_dev; a.theta = (double*)theta_dev;
  a.tbar = (double*)tbar_dev; a.state = (double*)state_dev; a.status = (int*)status_dev;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(gps_prep_kernel, dim3(1), dim3(256), 0, st, a);
  hipLaunchKernelGGL(gps_draw_kernel, dim3((D + 63) / 64, (S + 1 + 15) / 16), dim3(256), 0, st, a);
  BCX_TRY(who, hipGetLastError());
  return BCX_OK;
}
