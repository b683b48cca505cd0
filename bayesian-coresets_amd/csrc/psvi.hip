// psvi.hip -- the pseudo-point gradient of the batch pseudocoreset (BatchPSVI: coreset/bpsvi.py:42-60 of the reference, with
// projector.py:19-27 and the family gradients of examples/common/model_lr.py:50-57, model_linreg.py:12-17, model_poiss.py:58-67).
//
// In every family the gradient of a point's log-likelihood with respect to the point is a scalar times the parameter:
//     glls[i, s, :] = c(i, s) * tth_s,   tth_s = theta_s (logistic, Poisson) or [theta_s, 1] (linear regression, dz = D + 1),
// with c from t = x_i . theta_s:  logistic  m = -t, c = e^m / (1 + e^m) for m < 100, else 1;
//                                 linreg    c = (y_i - t) / sigsq;
//                                 Poisson   s = log(max(t, 0) + log1p(e^-|t|)) for t > -100, else t;
//                                           c = (y_i e^-s - 1)(1 - e^-e^s) where e^s > 1e-15, else y_i - e^s.
// projector.py:26 centres glls over its LAST axis (the coordinates of the point), so the centred gradient is
//     c(i, s) (tth_s - mean_j tth_s[j])
// and the pseudo-point gradient of one ADAM step, bpsvi.py:51-55,
//     ugrad = -diag(w) / S . (C o 1 resid^T) . Tc,      Tc[s, :] = tth_s - mean_j tth_s[j]
// is two products of k x S x D; the k x S x dz tensor of the reference is never formed.
//
//   psvi_prep_kernel   resid = scaling colsum - w^T corevecs (bpsvi.py:50) and the coordinate means of tth_s
//   psvi_wgrad_kernel  wgrad = -corevecs resid / S (bpsvi.py:51)
//   psvi_coef_kernel   P[:, :D] Theta^T on v_mfma_f64_16x16x4_f64 (operands from global memory as proj.hip's 32 x 32-block
//                      kernel stages them), the family's coefficient in the epilogue, times resid[s] (or not: the gradient write)
//   psvi_ugrad_kernel  (C o resid) . Tc on v_mfma_f64_16x16x4_f64, Tc formed as the operand is read, times -w_i / S
//   psvi_gwrite_kernel the centred k x S x dz gradients themselves (project(P, grad=True)): memory bound
// PS_GAUSSIAN (the Gaussian-mean family, model_gaussian.py:12-15) does not have that shape: grad_x loglik = Siginv theta_s - Siginv x_i
// is a DIFFERENCE of a term of the draw and a term of the point.  With g_s = Siginv (theta_s - tbar) (the projection's operand,
// csrc/gauss.hip) and h_i = Siginv (p_i - tbar) it is g_s - h_i, and centred over the coordinates
//     glls[i, s, :] = (g_s - mean_j g_s) - (h_i - mean_j h_i),
//     ugrad[i, :]   = -(w_i / S) ( sum_s resid_s (g_s - mean_j g_s)  -  (sum_s resid_s) (h_i - mean_j h_i) ):
// the first term does not depend on the point -- one S x D product with a vector, no k x S x D work at all.
//   psvi_gauss_gwrite_kernel / psvi_gauss_ugrad_kernel; own entry points (they take h, not the points).
// Every sum has one fixed order and no atomics: the results are the same bit for bit from run to run.  The coefficients use
// the device libm (exp / log / log1p): there are k x S of them, not N x S, so the table forms of proj_math.h save nothing
// measurable here, and the libm forms stay closer to NumPy's.
#include <string>
#include "bcx_internal.h"
#include "dev_util.h"
#include "launch_host.h"

enum { PS_LOGISTIC = 0, PS_POISSON = 1, PS_LINREG = 2, PS_GAUSSIAN = 3 };


typedef double ps4d __attribute__((ext_vector_type(4)));

template <int FAM>
static __device__ __forceinline__ double psvi_coef(double t, double y, double rsig) {
  if (FAM == PS_LOGISTIC) {                                    // model_lr.py:52-56
    const double m = -t;
    if (m < 100.0) {
      const double e = exp(m);
      return e / (1.0 + e);
    }
    return 1.0;
  } else if (FAM == PS_POISSON) {                              // model_poiss.py:36-41 (compute_s), 62-66
    double s = t;
    if (s > -100.0) s = log(fmax(s, 0.0) + log1p(exp(-fabs(s))));
    const double es = exp(s);
    if (es > 1e-15) return (y * exp(-s) - 1.0) * (1.0 - exp(-es));
    return y - es;
  } else {                                                     // model_linreg.py:17
    return rsig * (y - t);
  }
}

// resid[s] = scaling colsum[s] - sum_i w_i cv[i, s] (cv == nullptr: resid untouched) and tmean[s] = mean_j tth_s[j].
// A workgroup takes 16 columns; its 16 row slices (i = slice mod 16) are summed in a fixed order.
__global__ __launch_bounds__(256) void psvi_prep_kernel(int k, int S, const double* __restrict__ colsum, double scaling,
                                                        const double* __restrict__ cv, int64_t ldcv, const double* __restrict__ w,
                                                        double* __restrict__ resid, const double* __restrict__ theta, int64_t ldt,
                                                        int D, int dz, double* __restrict__ tmean) {
  __shared__ double part[16][17];
  const int c = threadIdx.x & 15, sl = threadIdx.x >> 4;
  const int s = blockIdx.x * 16 + c;
  double acc = 0.0;
  if (cv && s < S) {
#pragma unroll 4
    for (int i = sl; i < k; i += 16) acc = fma(w[i], cv[(int64_t)i * ldcv + s], acc);
  }
  part[sl][c] = acc;
  double m = 0.0;
  if (sl == 1 && s < S) {                                      // (another slice than the one that combines below)
    const double* tp = theta + (int64_t)s * ldt;
    for (int j = 0; j < D; ++j) m += tp[j];
    if (dz > D) m += 1.0;
    tmean[s] = m / (double)dz;
  }
  __syncthreads();
  if (sl == 0 && cv && s < S) {
    double t = part[0][c];
    for (int q = 1; q < 16; ++q) t += part[q][c];
    resid[s] = scaling * colsum[s] - t;
  }
}

// wgrad[i] = -(cv[i, :] . resid) / S, one workgroup per row
__global__ __launch_bounds__(256) void psvi_wgrad_kernel(int S, const double* __restrict__ cv, int64_t ldcv,
                                                         const double* __restrict__ resid, double* __restrict__ wgrad) {
  __shared__ double scratch[BCX_SCRATCH];
  const double* row = cv + (int64_t)blockIdx.x * ldcv;
  double v[1] = {0.0};
  for (int s = threadIdx.x; s < S; s += 256) v[0] = fma(row[s], resid[s], v[0]);
  block_allsum<1>(v, scratch);
  if (threadIdx.x == 0) wgrad[blockIdx.x] = -v[0] / (double)S;
}

// C[i, s] = c(i, s) (* resid[s]) for a 32 x 32 block per workgroup, one 16 x 16 tile per wave.  Lane (li = lane % 16,
// lk = lane / 16) feeds row li's values 8 lk .. 8 lk + 7 of each run of 32 of the inner dimension, one per MFMA step (both
// operands take the inner index in the same order).  Accumulator register r: (row lk + 4 r, column li) of the wave's tile.
template <int FAM>
__global__ __launch_bounds__(256) void psvi_coef_kernel(const double* __restrict__ P, int k, int64_t ldp, int D, int ycol,
                                                        const double* __restrict__ theta, int S, int64_t ldt, double rsig,
                                                        const double* __restrict__ resid, double* __restrict__ C) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int li = lane & 15, lk = lane >> 4, rb = wave >> 1, cb = wave & 1;
  const int arow = blockIdx.x * 32 + rb * 16 + li, bcol = blockIdx.y * 32 + cb * 16 + li;
  const bool aok = arow < k, bok = bcol < S;
  const double* ap = P + (int64_t)(aok ? arow : 0) * ldp;
  const double* bp = theta + (int64_t)(bok ? bcol : 0) * ldt;
  ps4d acc = (ps4d){0.0, 0.0, 0.0, 0.0};
  for (int kb = 0; kb < D; kb += 32) {
    double xa[8], xb[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int kk = kb + 8 * lk + q;
      const bool ok = kk < D;
      const double a = ap[ok ? kk : 0], b = bp[ok ? kk : 0];
      xa[q] = (ok && aok) ? a : 0.0;
      xb[q] = (ok && bok) ? b : 0.0;
    }
#pragma unroll
    for (int t = 0; t < 8; ++t) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(xa[t], xb[t], acc, 0, 0, 0);
  }
  const int col = bcol;
  const double rs = (resid && bok) ? resid[col] : 1.0;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = blockIdx.x * 32 + rb * 16 + lk + 4 * r;
    if (row < k && bok) {
      const double y = FAM == PS_LOGISTIC ? 0.0 : P[(int64_t)row * ldp + ycol];
      const double c = psvi_coef<FAM>(acc[r], y, rsig);
      C[(int64_t)row * S + col] = resid ? c * rs : c;
    }
  }
}

// ugrad[i, j] = -(w_i sum_s C[i, s] (tth_s[j] - tmean[s])) / S for j < dz: the same block / lane shape, inner index s
template <bool LIN>
__global__ __launch_bounds__(256) void psvi_ugrad_kernel(const double* __restrict__ C, int k, int S,
                                                         const double* __restrict__ theta, int64_t ldt, int D, int dz,
                                                         const double* __restrict__ tmean, const double* __restrict__ w,
                                                         double* __restrict__ U) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int li = lane & 15, lk = lane >> 4, rb = wave >> 1, cb = wave & 1;
  const int arow = blockIdx.x * 32 + rb * 16 + li, bcol = blockIdx.y * 32 + cb * 16 + li;
  const bool aok = arow < k, bok = bcol < dz, one = LIN && bcol == D;
  const double* ap = C + (int64_t)(aok ? arow : 0) * S;
  const double* bp = theta + (bcol < D ? bcol : 0);
  ps4d acc = (ps4d){0.0, 0.0, 0.0, 0.0};
  for (int sb = 0; sb < S; sb += 32) {
    double xa[8], xb[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int s = sb + 8 * lk + q;
      const bool ok = s < S;
      const int sc = ok ? s : 0;
      const double a = ap[sc], th = bp[(int64_t)sc * ldt], m = tmean[sc];
      xa[q] = (ok && aok) ? a : 0.0;
      xb[q] = (ok && bok) ? (one ? 1.0 : th) - m : 0.0;
    }
#pragma unroll
    for (int t = 0; t < 8; ++t) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(xa[t], xb[t], acc, 0, 0, 0);
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = blockIdx.x * 32 + rb * 16 + lk + 4 * r;
    if (row < k && bok) U[(int64_t)row * dz + bcol] = -(w[row] * acc[r]) / (double)S;
  }
}

// G[i, s, j] = C[i, s] (tth_s[j] - tmean[s]), k x S x dz, row-major
template <bool LIN>
__global__ __launch_bounds__(256) void psvi_gwrite_kernel(const double* __restrict__ C, int S, const double* __restrict__ theta,
                                                          int64_t ldt, int D, int dz, const double* __restrict__ tmean,
                                                          double* __restrict__ G, int64_t total) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) {
    const int64_t row = e / dz;                                // i S + s
    const int j = (int)(e - row * dz), s = (int)(row % S);
    const double th = (LIN && j == D) ? 1.0 : theta[(int64_t)s * ldt + (j < D ? j : 0)];
    G[e] = C[row] * (th - tmean[s]);
  }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------
// the checks both entries share; *dz: the length of a gradient row
static int ps_check(const char* who, int32_t family, const void* P, int32_t k, int64_t ldp, int32_t D, int32_t ycol,
                    const void* theta, int32_t S, int64_t ldt, double param, const void* work, int* dz) {
  if (family == PS_GAUSSIAN) return bcx_fail(BCX_ERR_ARG, who, "family 3 (Gaussian mean) has entry points of its own: bcx_project_grad_points_gaussian / bcx_psvi_gradient_gaussian");
  if (family < PS_LOGISTIC || family > PS_LINREG) return bcx_fail(BCX_ERR_ARG, who, "unknown likelihood family");
  if (k < 1 || k > BCX_PSVI_MAX_POINTS) return bcx_fail(BCX_ERR_ARG, who, "k (pseudo-points) must be in 1 .. 4096");
  if (S < 1 || S > BCX_PSVI_MAX_SAMPLES) return bcx_fail(BCX_ERR_ARG, who, "S (samples) must be in 1 .. 8192");
  if (D < 1 || D > BCX_PSVI_MAX_DIM) return bcx_fail(BCX_ERR_ARG, who, "D (features) must be in 1 .. 1024");
  if (!P || !theta || !work) return bcx_fail(BCX_ERR_ARG, who, "null pointer");
  if (ldp < D || ldt < D) return bcx_fail(BCX_ERR_ARG, who, "leading dimension shorter than D");
  if (family != PS_LOGISTIC && (ycol < 0 || ycol >= ldp)) return bcx_fail(BCX_ERR_ARG, who, "response column required");
  if (family == PS_LINREG && !(param != 0.0)) return bcx_fail(BCX_ERR_ARG, who, "sigsq must be non-zero");
  *dz = family == PS_LINREG ? D + 1 : D;
  return BCX_OK;
}

static int ps_coef(const char* who, hipStream_t st, int32_t family, const double* P, int k, int64_t ldp, int D, int ycol, const double* theta, int S,
                   int64_t ldt, double param, const double* resid, double* C) {
  const dim3 grid((k + 31) / 32, (S + 31) / 32);
  const double rsig = family == PS_LINREG ? 1.0 / param : 0.0;
  if (family == PS_LOGISTIC)
    hipLaunchKernelGGL(psvi_coef_kernel<PS_LOGISTIC>, grid, dim3(256), 0, st, P, k, ldp, D, ycol, theta, S, ldt, rsig, resid, C);
  else if (family == PS_POISSON)
    hipLaunchKernelGGL(psvi_coef_kernel<PS_POISSON>, grid, dim3(256), 0, st, P, k, ldp, D, ycol, theta, S, ldt, rsig, resid, C);
  else
    hipLaunchKernelGGL(psvi_coef_kernel<PS_LINREG>, grid, dim3(256), 0, st, P, k, ldp, D, ycol, theta, S, ldt, rsig, resid, C);
  BCX_TRY(who, hipGetLastError());
  return BCX_OK;
}

extern "C" int64_t bcx_psvi_gradient_scratch_bytes(int32_t k, int32_t S) {
  if (k < 1 || k > BCX_PSVI_MAX_POINTS || S < 1 || S > BCX_PSVI_MAX_SAMPLES) return -1;
  return ((int64_t)k * S + S) * (int64_t)sizeof(double);
}

extern "C" int bcx_project_grad_points(void* stream, int32_t family, const void* P_dev, int32_t k, int64_t ldp, int32_t D,
                                       int32_t ycol, const void* theta_dev, int32_t S, int32_t ldt, double param, void* glls_dev,
                                       void* work_dev) {
  static const char* who = "bcx_project_grad_points";
  int dz = 0;
  int rc = ps_check(who, family, P_dev, k, ldp, D, ycol, theta_dev, S, ldt, param, work_dev, &dz);
  if (rc) return rc;
  if (!glls_dev) return bcx_fail(BCX_ERR_ARG, who, "null output");
  hipStream_t st = (hipStream_t)stream;
  const double* P = (const double*)P_dev;
  const double* theta = (const double*)theta_dev;
  double* C = (double*)work_dev;
  double* tmean = C + (int64_t)k * S;
  hipLaunchKernelGGL(psvi_prep_kernel, dim3((S + 15) / 16), dim3(256), 0, st, k, S, (const double*)nullptr, 0.0,
                     (const double*)nullptr, (int64_t)0, (const double*)nullptr, (double*)nullptr, theta, (int64_t)ldt, D, dz, tmean);
  BCX_TRY(who, hipGetLastError());
  rc = ps_coef(who, st, family, P, k, ldp, D, ycol, theta, S, ldt, param, nullptr, C);
  if (rc) return rc;
  const int64_t total = (int64_t)k * S * dz;
  const int64_t want = (total + 255) / 256;
  const int blocks = (int)(want < 8192 ? want : 8192);
  if (family == PS_LINREG)
    hipLaunchKernelGGL(psvi_gwrite_kernel<true>, dim3(blocks), dim3(256), 0, st, C, S, theta, (int64_t)ldt, D, dz, tmean,
                       (double*)glls_dev, total);
  else
    hipLaunchKernelGGL(psvi_gwrite_kernel<false>, dim3(blocks), dim3(256), 0, st, C, S, theta, (int64_t)ldt, D, dz, tmean,
                       (double*)glls_dev, total);
  BCX_TRY(who, hipGetLastError());
  return BCX_OK;
}

extern "C" int bcx_psvi_gradient(void* stream, int32_t family, const void* P_dev, int32_t k, int64_t ldp, int32_t D, int32_t ycol,
                                 const void* theta_dev, int32_t S, int32_t ldt, double param, const void* colsum_dev,
                                 const void* corevecs_dev, int64_t ldcv, const void* w_dev, double scaling, void* out_dev,
                                 void* work_dev) {
  static const char* who = "bcx_psvi_gradient";
  int dz = 0;
  int rc = ps_check(who, family, P_dev, k, ldp, D, ycol, theta_dev, S, ldt, param, work_dev, &dz);
  if (rc) return rc;
  if (!colsum_dev || !corevecs_dev || !w_dev || !out_dev) return bcx_fail(BCX_ERR_ARG, who, "null pointer");
  if (ldcv < S) return bcx_fail(BCX_ERR_ARG, who, "corevecs leading dimension shorter than S");
  hipStream_t st = (hipStream_t)stream;
  const double* P = (const double*)P_dev;
  const double* theta = (const double*)theta_dev;
  const double* cv = (const double*)corevecs_dev;
  const double* w = (const double*)w_dev;
  double* resid = (double*)out_dev;
  double* wgrad = resid + S;
  double* ugrad = wgrad + k;
  double* A = (double*)work_dev;
  double* tmean = A + (int64_t)k * S;
  hipLaunchKernelGGL(psvi_prep_kernel, dim3((S + 15) / 16), dim3(256), 0, st, k, S, (const double*)colsum_dev, scaling, cv, ldcv, w,
                     resid, theta, (int64_t)ldt, D, dz, tmean);
  BCX_TRY(who, hipGetLastError());
  hipLaunchKernelGGL(psvi_wgrad_kernel, dim3(k), dim3(256), 0, st, S, cv, ldcv, (const double*)resid, wgrad);
  BCX_TRY(who, hipGetLastError());
  rc = ps_coef(who, st, family, P, k, ldp, D, ycol, theta, S, ldt, param, resid, A);
  if (rc) return rc;
  const dim3 grid((k + 31) / 32, (dz + 31) / 32);
  if (family == PS_LINREG)
    hipLaunchKernelGGL(psvi_ugrad_kernel<true>, grid, dim3(256), 0, st, (const double*)A, k, S, theta, (int64_t)ldt, D, dz,
                       (const double*)tmean, w, ugrad);
  else
    hipLaunchKernelGGL(psvi_ugrad_kernel<false>, grid, dim3(256), 0, st, (const double*)A, k, S, theta, (int64_t)ldt, D, dz,
                       (const double*)tmean, w, ugrad);
  BCX_TRY(who, hipGetLastError());
  return BCX_OK;
}

// ---- PS_GAUSSIAN -----------------------------------------------------------------------------------------------------------------------
// G[i, s, j] = (g_s[j] - gmean[s]) - (H[i][j] - H[i][D]),  k x S x D row-major.  H[i][D]: the mean of row i's coordinates (csrc/gauss.hip).
__global__ __launch_bounds__(256) void psvi_gauss_gwrite_kernel(const double* __restrict__ op, int64_t ldt, const double* __restrict__ gmean,
                                                                const double* __restrict__ H, int64_t ldh, int S, int D,
                                                                double* __restrict__ G, int64_t total) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) {
    const int64_t row = e / D;                                 // i S + s
    const int j = (int)(e - row * D), s = (int)(row % S);
    const int64_t i = row / S;
    G[e] = (op[(int64_t)s * ldt + j] - gmean[s]) - (H[i * ldh + j] - H[i * ldh + D]);
  }
}

// U[i, j] = -(w_i / S) (v_j - rs (H[i][j] - H[i][D])),  v_j = sum_s resid_s (g_s[j] - gmean[s]),  rs = sum_s resid_s.
// A workgroup takes 64 coordinates: thread (c = tid % 64, q = tid / 64) sums the samples q, q + 4, ...; the four classes are added 0..3.
__global__ __launch_bounds__(256) void psvi_gauss_ugrad_kernel(const double* __restrict__ op, int64_t ldt, const double* __restrict__ gmean,
                                                               const double* __restrict__ resid, const double* __restrict__ H, int64_t ldh,
                                                               const double* __restrict__ w, int k, int S, int D, double* __restrict__ U) {
  __shared__ double seg[4][64], rseg[4];
  const int c = threadIdx.x & 63, q = threadIdx.x >> 6, j = blockIdx.x * 64 + c;
  double acc = 0.0, racc = 0.0;
  for (int s = q; s < S; s += 4) {
    const double r = resid[s];
    racc += r;
    if (j < D) acc = fma(r, op[(int64_t)s * ldt + j] - gmean[s], acc);
  }
  seg[q][c] = acc;
  if (c == 0) rseg[q] = racc;
  __syncthreads();
  if (j >= D) return;
  const double v = ((seg[0][c] + seg[1][c]) + seg[2][c]) + seg[3][c];
  const double rs = ((rseg[0] + rseg[1]) + rseg[2]) + rseg[3];
  for (int i = q; i < k; i += 4) {
    const double* h = H + (int64_t)i * ldh;
    U[(int64_t)i * D + j] = -(w[i] * (v - rs * (h[j] - h[D]))) / (double)S;
  }
}

static int ps_gauss_check(const char* who, const void* op, int32_t S, int64_t ldt, int32_t D, const void* H, int32_t k, int64_t ldh,
                          const void* work) {
  if (k < 1 || k > BCX_PSVI_MAX_POINTS) return bcx_fail(BCX_ERR_ARG, who, "k (pseudo-points) must be in 1 .. 4096");
  if (S < 1 || S > BCX_PSVI_MAX_SAMPLES) return bcx_fail(BCX_ERR_ARG, who, "S (samples) must be in 1 .. 8192");
  if (D < 1 || D > BCX_PSVI_MAX_DIM) return bcx_fail(BCX_ERR_ARG, who, "D (coordinates) must be in 1 .. 1024");
  if (!op || !H || !work) return bcx_fail(BCX_ERR_ARG, who, "null pointer");
  if (ldt < D + 1 || ldh < D + 1) return bcx_fail(BCX_ERR_ARG, who, "operands of bcx_gaussian_operand required (leading dimensions >= D + 1)");
  return BCX_OK;
}

extern "C" int bcx_project_grad_points_gaussian(void* stream, const void* operand_dev, int32_t S, int64_t ldt, int32_t D, const void* H_dev,
                                                int32_t k, int64_t ldh, void* glls_dev, void* work_dev) {
  static const char* who = "bcx_project_grad_points_gaussian";
  int rc = ps_gauss_check(who, operand_dev, S, ldt, D, H_dev, k, ldh, work_dev);
  if (rc) return rc;
  if (!glls_dev) return bcx_fail(BCX_ERR_ARG, who, "null output");
  hipStream_t st = (hipStream_t)stream;
  const double* op = (const double*)operand_dev;
  double* gmean = (double*)work_dev + (int64_t)k * S;       // (the place the other families keep it: same scratch size)
  hipLaunchKernelGGL(psvi_prep_kernel, dim3((S + 15) / 16), dim3(256), 0, st, k, S, (const double*)nullptr, 0.0,
                     (const double*)nullptr, (int64_t)0, (const double*)nullptr, (double*)nullptr, op, ldt, D, D, gmean);
  BCX_TRY(who, hipGetLastError());
  const int64_t total = (int64_t)k * S * D;
  const int64_t want = (total + 255) / 256;
  const int blocks = (int)(want < 8192 ? want : 8192);
  hipLaunchKernelGGL(psvi_gauss_gwrite_kernel, dim3(blocks), dim3(256), 0, st, op, ldt, (const double*)gmean, (const double*)H_dev, ldh,
                     (int)S, (int)D, (double*)glls_dev, total);
  BCX_TRY(who, hipGetLastError());
  return BCX_OK;
}

extern "C" int bcx_psvi_gradient_gaussian(void* stream, const void* operand_dev, int32_t S, int64_t ldt, int32_t D, const void* H_dev,
                                          int32_t k, int64_t ldh, const void* colsum_dev, const void* corevecs_dev, int64_t ldcv,
                                          const void* w_dev, double scaling, void* out_dev, void* work_dev) {
  static const char* who = "bcx_psvi_gradient_gaussian";
  int rc = ps_gauss_check(who, operand_dev, S, ldt, D, H_dev, k, ldh, work_dev);
  if (rc) return rc;
  if (!colsum_dev || !corevecs_dev || !w_dev || !out_dev) return bcx_fail(BCX_ERR_ARG, who, "null pointer");
  if (ldcv < S) return bcx_fail(BCX_ERR_ARG, who, "corevecs leading dimension shorter than S");
  hipStream_t st = (hipStream_t)stream;
  const double* op = (const double*)operand_dev;
  const double* cv = (const double*)corevecs_dev;
  const double* w = (const double*)w_dev;
  double* resid = (double*)out_dev;
  double* wgrad = resid + S;
  double* ugrad = wgrad + k;
  double* gmean = (double*)work_dev + (int64_t)k * S;
  hipLaunchKernelGGL(psvi_prep_kernel, dim3((S + 15) / 16), dim3(256), 0, st, k, S, (const double*)colsum_dev, scaling, cv, ldcv, w,
                     resid, op, ldt, D, D, gmean);
  BCX_TRY(who, hipGetLastError());
  hipLaunchKernelGGL(psvi_wgrad_kernel, dim3(k), dim3(256), 0, st, S, cv, ldcv, (const double*)resid, wgrad);
  BCX_TRY(who, hipGetLastError());
  hipLaunchKernelGGL(psvi_gauss_ugrad_kernel, dim3((D + 63) / 64), dim3(256), 0, st, op, ldt, (const double*)gmean, (const double*)resid,
                     (const double*)H_dev, ldh, w, (int)k, (int)S, (int)D, ugrad);
  BCX_TRY(who, hipGetLastError());
  return BCX_OK;
}

// ---- the ADAM step of BatchPSVI's device-resident loop ---------------------------------------------------------------------------
// One step of nn_opt (util/opt.py:15-23) on x = [w (k) | P (k x d)] with nn_idcs = arange(k) (bpsvi.py:57-60): elementwise,
//     m1 = b1 m1 + (1 - b1) g,  m2 = b2 m2 + (1 - b2) g^2,  x -= step m1 / c1 / (eps + sqrt(m2 / c2)),  w = max(w, 0) (a NaN stays)
// with g read where bcx_psvi_gradient left it ([resid (S) | wgrad (k) | ugrad (k x d)]) and (step, c1, c2) = sched[3 i ..].
// A workgroup takes 32 rows x 16 columns of P; lane (r = lane % 8, c = lane / 8) of wave v takes row 8 v + r, columns 2 c, 2 c + 1:
// eight lanes read 128 adjacent bytes of a row (one 16-byte load each from P, m1, m2; from g too where its address allows --
// the gradient rows are d doubles apart, not ldp), and the mirror for the linreg sampler's D x D form (XT: features BY points,
// ldk apart; y: the last column) receives, for one column, the 8 adjacent rows of a wave as 64 adjacent bytes.  The workgroups of
// the first column block also step the 32 weights of their rows.  Every load of a thread is issued before its arithmetic; no
// LDS, no atomics.  The moments are laid out as the state is: [k weights, padded to even | k x ldp].
struct PsaArgs {
  const double* g; const double* sched;
  double* w; double* P; double* m1; double* m2; double* XT; double* y; double* trace;
  int64_t ldp, ldk;
  int k, d, S, step;
  double b1, b2, eps;
};

typedef double ps2d __attribute__((ext_vector_type(2)));

static __device__ __forceinline__ double psa_step(double x, double g, double& m1, double& m2, double b1, double b2, double eps,
                                                  double stp, double c1, double c2) {
  m1 = b1 * m1 + (1.0 - b1) * g;
  m2 = b2 * m2 + (1.0 - b2) * (g * g);
  return x - stp * m1 / c1 / (eps + sqrt(m2 / c2));
}

__global__ __launch_bounds__(256) void psvi_adam_kernel(PsaArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = blockIdx.y * 32 + wave * 8 + (lane & 7), j = blockIdx.x * 16 + 2 * (lane >> 3);
  const int k = a.k, d = a.d;
  if (i >= k || j >= d) return;
  const bool two = j + 1 < d, wt = j == 0;
  const int64_t kq = (int64_t)k + (k & 1);
  const int64_t po = (int64_t)i * a.ldp + j, go = (int64_t)a.S + k + (int64_t)i * d + j;
  // loads
  const ps2d x = *(const ps2d*)(a.P + po);                       // (d odd: the second value of the last pair is the row's padding)
  const ps2d m1v = *(const ps2d*)(a.m1 + kq + po), m2v = *(const ps2d*)(a.m2 + kq + po);
  double g0, g1 = 0.0;
  if (two && (((uintptr_t)(a.g + go)) & 15) == 0) {
    const ps2d gv = *(const ps2d*)(a.g + go);
    g0 = gv[0]; g1 = gv[1];
  } else {
    g0 = a.g[go];
    if (two) g1 = a.g[go + 1];
  }
  double xw = 0.0, gw = 0.0, mw1 = 0.0, mw2 = 0.0;
  if (wt) { xw = a.w[i]; gw = a.g[a.S + i]; mw1 = a.m1[i]; mw2 = a.m2[i]; }
  const double* sc = a.sched + 3 * (int64_t)a.step;
  const double stp = sc[0], c1 = sc[1], c2 = sc[2];
  // arithmetic
  double n1a = m1v[0], n2a = m2v[0], n1b = m1v[1], n2b = m2v[1];
  const double xa = psa_step(x[0], g0, n1a, n2a, a.b1, a.b2, a.eps, stp, c1, c2);
  double xb = x[1];
  if (two) xb = psa_step(x[1], g1, n1b, n2b, a.b1, a.b2, a.eps, stp, c1, c2);
  // stores
  if (two) {
    *(ps2d*)(a.P + po) = (ps2d){xa, xb};
    *(ps2d*)(a.m1 + kq + po) = (ps2d){n1a, n1b};
    *(ps2d*)(a.m2 + kq + po) = (ps2d){n2a, n2b};
  } else {
    a.P[po] = xa; a.m1[kq + po] = n1a; a.m2[kq + po] = n2a;
  }
  if (a.XT) {                                                    // columns 0 .. d - 2 are the features, d - 1 the response
    if (j < d - 1) a.XT[(int64_t)j * a.ldk + i] = xa; else a.y[i] = xa;
    if (two) { if (j + 1 < d - 1) a.XT[(int64_t)(j + 1) * a.ldk + i] = xb; else a.y[i] = xb; }
  }
  double* tr = a.trace ? a.trace + (int64_t)a.step * ((int64_t)k * (1 + d)) : nullptr;
  if (tr) {
    tr[(int64_t)k + (int64_t)i * d + j] = xa;
    if (two) tr[(int64_t)k + (int64_t)i * d + j + 1] = xb;
  }
  if (wt) {
    const double xn = bcx_clamp0(psa_step(xw, gw, mw1, mw2, a.b1, a.b2, a.eps, stp, c1, c2));
    a.w[i] = xn; a.m1[i] = mw1; a.m2[i] = mw2;
    if (tr) tr[i] = xn;
  }
}

extern "C" int bcx_psvi_adam_step(void* stream, int32_t k, int32_t d, const void* grad_dev, int32_t S, void* w_dev, void* P_dev,
                                  int64_t ldp, void* mom1_dev, void* mom2_dev, const void* sched_dev, int32_t step, double b1,
                                  double b2, double eps, void* XT_dev, int64_t ldk, void* y_dev, void* trace_dev) {
  static const char* who = "bcx_psvi_adam_step";
  if (k < 1 || k > BCX_PSVI_MAX_POINTS) return bcx_fail(BCX_ERR_ARG, who, "k (pseudo-points) must be in 1 .. 4096");
  if (d < 1 || d > BCX_PSVI_ADAM_MAX_COLS) return bcx_fail(BCX_ERR_ARG, who, "d (columns of a point) must be in 1 .. 4096");
  if (S < 1 || S > BCX_PSVI_MAX_SAMPLES) return bcx_fail(BCX_ERR_ARG, who, "S (samples) must be in 1 .. 8192");
  if (step < 0) return bcx_fail(BCX_ERR_ARG, who, "step must not be negative");
  if (!grad_dev || !w_dev || !P_dev || !mom1_dev || !mom2_dev || !sched_dev) return bcx_fail(BCX_ERR_ARG, who, "null pointer");
  if (ldp < d || (ldp & 1)) return bcx_fail(BCX_ERR_ARG, who, "ldp must be even and at least d (rows of the points start on 16-byte boundaries)");
  if (((uintptr_t)P_dev | (uintptr_t)mom1_dev | (uintptr_t)mom2_dev) & 15) return bcx_fail(BCX_ERR_ARG, who, "points and moments must be 16-byte aligned");
  if (((uintptr_t)grad_dev | (uintptr_t)w_dev | (uintptr_t)sched_dev | (uintptr_t)trace_dev) & 7) return bcx_fail(BCX_ERR_ARG, who, "misaligned pointer");
  if (XT_dev) {
    if (!y_dev) return bcx_fail(BCX_ERR_ARG, who, "the mirror needs both XT and y");
    if (d < 2) return bcx_fail(BCX_ERR_ARG, who, "the mirror needs a feature and the response (d >= 2)");
    if (ldk < ((int64_t)k + 31) / 32 * 32) return bcx_fail(BCX_ERR_ARG, who, "ldk must be at least k rounded up to 32");
    if (((uintptr_t)XT_dev | (uintptr_t)y_dev) & 7) return bcx_fail(BCX_ERR_ARG, who, "misaligned pointer");
  }
  PsaArgs a;
  a.g = (const double*)grad_dev; a.sched = (const double*)sched_dev;
  a.w = (double*)w_dev; a.P = (double*)P_dev; a.m1 = (double*)mom1_dev; a.m2 = (double*)mom2_dev;
  a.XT = (double*)XT_dev; a.y = (double*)y_dev; a.trace = (double*)trace_dev;
  a.ldp = ldp; a.ldk = ldk; a.k = k; a.d = d; a.S = S; a.step = step; a.b1 = b1; a.b2 = b2; a.eps = eps;
  hipLaunchKernelGGL(psvi_adam_kernel, dim3((d + 15) / 16, (k + 31) / 32), dim3(256), 0, (hipStream_t)stream, a);
  BCX_TRY(who, hipGetLastError());
  return BCX_OK;
}
