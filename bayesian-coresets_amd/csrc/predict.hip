// predict.hip -- the log predictive density of held-out rows under posterior draws, the metric the Hilbert-coreset experiments
// report next to the moment errors: for a row z_n and draws theta_1 .. theta_S
//     lppd[n] = log( 1/S sum_s p(z_n | theta_s) ) = logsumexp_s ll(z_n, theta_s) - log S,      mean[n] = 1/S sum_s ll(z_n, theta_s)
// with ll the reference's full log-likelihood (model_lr.py:25-32; model_poiss.py:25-38, the Poisson -log y! included).  It is
// the N x S table bcx_log_joint_grad (csrc/hmc.hip) sums over the rows, reduced the other way -- and never stored:
//
//   pred_rows_kernel     a workgroup owns 128 rows and one contiguous range of the draws.  The products x_n . theta_s run on
//                        v_mfma_f64_16x16x4_f64 with the DRAWS on the M side and the ROWS on the N side: the accumulator of lane
//                        (li = lane % 16, lk = lane / 16) holds draws s0 + lk + 4 r (r = 0..3) of row li, so the online
//                        log-sum-exp -- a running maximum m, sum exp(ll - m), sum ll -- is serial per lane with no cross-lane
//                        traffic in the loop.  A wave carries two such row tiles (32 rows) against one read of the draws.  The
//                        row operand (k = 4 t + lk of row li, zero beyond D) stays in registers for the whole range; the draw
//                        operand of the next 16 draws is read while the likelihood of the current ones runs.  At the end the
//                        four lanes of a row are merged in lane order and one record (m, sum, sum ll) per (range, row) written.
//   pred_combine_kernel  one thread per row: the ranges' records merged in range order, lppd = m + log(sum / S), mean = sum ll / S.
//
// The likelihood and the exponential of the log-sum-exp are csrc/proj_math.h's table forms (exp on x <= 0, log1p on [0, 1], log
// of a positive number: 11, 10 and 12 fp64 instructions, <= 1.5 ulp; the tables in LDS), the forms of proj.hip's epilogues.
// csrc/lik_point.h's libm form -- the text of the samplers, which tests/test_gpu_predictive.py holds this one to through
// bc.log_joint_grad -- was measured first and took 2 - 2.4 times as long.  No floating-point atomics, every
// order fixed: two calls give the same bits.  A NaN anywhere in a row's table makes sum ll NaN, which makes both outputs of
// that row NaN; the maximum is formed by comparisons that a NaN never wins, and exp(NaN - m) poisons the sum besides.
// ll = -inf (a draw of probability zero) contributes an exact zero; a row whose every ll is -inf comes out as -inf.
//
// Bound: the fp64 VALU epilogue -- two exponentials and one log1p (Poisson: a log besides) per value against
// 2 D flops of product on the matrix pipe, which shares the datapath (proj_math.h).
#include <math.h>
#include <string>
#include "bcx_internal.h"
#include "lik_point.h"
#include "proj_math.h"
#include "launch_host.h"

#define PRED_DMAX 32
#define PRED_ROWS 128            // rows of a workgroup: 4 waves x 2 tiles of 16
#define PRED_KSTEPS 8            // MFMA steps of 4 for D <= 32
#define PRED_MAX_SPLITS 4096
#define PRED_MIN_RANGE 256       // the library's own choice keeps a range at least this long

typedef double pred4d __attribute__((ext_vector_type(4)));
typedef const double __attribute__((address_space(3)))* pred_tab_t;

struct PredArgs {
  const double* Z;      // N x ldz rows (logistic: y x; Poisson: [x, y])
  const double* Th;     // S x ldt draws
  const double* tab;    // the tables of proj_math.h (proj_tables())
  double* rec;          // splits x N x 3: (m, sum exp(ll - m), sum ll) of a range of the draws
  int64_t N, ldz, S, ldt;
  int D, splits;
};

// (m, s, l) += (m2, s2, l2): two partial log-sum-exps in this order.  m is never NaN (only `>` moves it); a part with
// m = -inf has s = 0 and adds nothing.
static __device__ __forceinline__ void pred_merge(double& m, double& s, double& l, double m2, double s2, double l2) {
  if (m2 > m) { s = s * exp(m - m2) + s2; m = m2; }
  else if (m2 > -INFINITY) s += s2 * exp(m2 - m);
  l += l2;
}

// ll of one (row, draw) from the linear predictor s; lg = log y! (Poisson).  proj.hip's loglik, term for term:
//   logistic  -log1p(exp(-s)) = min(s, 0) - log1p(exp(-|s|)), which IS s to every bit from -s = 100 on (model_lr.py:29-31)
//   Poisson   rate = max(s, 0) + log1p(exp(-|s|)), y log(rate) - rate - log y!, log(rate) = s from s = -100 down
//             (model_poiss.py:25-38; exp(log(rate)) is the rate itself)
// s = +-inf gives the limit (logistic 0 / -inf, Poisson -inf, or NaN where the limit is 0 x inf), a NaN a NaN.
template <int FAM> static __device__ __forceinline__ double pred_ll(double s, double y, double lg, pred_tab_t tab) {
  const double soft = pjm_log1p01(pjm_exp_nonpos(-fabs(s), tab), tab);
  if (FAM == LAP_LOGISTIC) return (pjm_hi(s) < 0 ? s : 0.0) - soft;
  const double rate = pjm_relu(s) + soft;
  const double lr = s > -100.0 ? pjm_log_pos(rate, tab) : s;
  return y * lr - lg - rate;
}

template <int FAM>
__global__ __launch_bounds__(256) void pred_rows_kernel(PredArgs a) {
  __shared__ __attribute__((aligned(16))) double s_tab[PJT_LFACT];
  for (int k = threadIdx.x; k < PJT_LFACT; k += 256) s_tab[k] = a.tab[k];
  const pred_tab_t tab = (pred_tab_t)s_tab;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int li = lane & 15, lk = lane >> 4;
  const int D = a.D, ksteps = (D + 3) >> 2;
  const int64_t row0 = (int64_t)blockIdx.x * PRED_ROWS + wave * 32;
  const int64_t s_begin = a.S * (int64_t)blockIdx.y / a.splits, s_end = a.S * ((int64_t)blockIdx.y + 1) / a.splits;

  // the row operand of both tiles, y and log y! of the lane's two rows: once per workgroup
  double xb[2][PRED_KSTEPS], y[2], lg[2];
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const int64_t row = row0 + 16 * c + li;
    const bool rok = row < a.N;
    const double* zp = a.Z + (rok ? row : 0) * a.ldz;
#pragma unroll
    for (int t = 0; t < PRED_KSTEPS; ++t) {
      const int kk = 4 * t + lk;
      const bool ok = rok && kk < D;
      const double v = zp[ok ? kk : 0];
      xb[c][t] = ok ? v : 0.0;
    }
    const double yy = (FAM == LAP_POISSON) ? zp[D] : 0.0;
    y[c] = (FAM == LAP_POISSON && rok) ? yy : 0.0;
    lg[c] = (FAM == LAP_POISSON) ? lgamma(y[c] + 1.0) : 0.0;
  }

  auto load_draws = [&](int64_t s0, double (&xa)[PRED_KSTEPS]) {
    const int64_t s = s0 + li;
    const bool sok = s < s_end;
    const double* tp = a.Th + (sok ? s : s_begin) * a.ldt;
#pragma unroll
    for (int t = 0; t < PRED_KSTEPS; ++t) {
      const int kk = 4 * t + lk;
      const bool ok = sok && kk < D;
      const double v = (t < ksteps) ? tp[ok ? kk : 0] : 0.0;
      xa[t] = ok ? v : 0.0;
    }
  };

  __syncthreads();                                     // (the tables)
  double m[2] = {-INFINITY, -INFINITY}, sum[2] = {0.0, 0.0}, sl[2] = {0.0, 0.0};
  double xa[PRED_KSTEPS];
  if (s_begin < s_end) load_draws(s_begin, xa);
  for (int64_t s0 = s_begin; s0 < s_end; s0 += 16) {
    pred4d acc[2] = {(pred4d){0.0, 0.0, 0.0, 0.0}, (pred4d){0.0, 0.0, 0.0, 0.0}};
#pragma unroll
    for (int t = 0; t < PRED_KSTEPS; ++t) {
      if (t < ksteps) {
        acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(xa[t], xb[0][t], acc[0], 0, 0, 0);
        acc[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(xa[t], xb[1][t], acc[1], 0, 0, 0);
      }
    }
    if (s0 + 16 < s_end) load_draws(s0 + 16, xa);      // (the next tile's operand, in flight under the likelihood)
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      double l[4];
      double mx = m[c];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const double ll = pred_ll<FAM>(acc[c][r], y[c], lg[c], tab);
        const bool ok = s0 + lk + 4 * r < s_end;
        sl[c] += ok ? ll : 0.0;
        l[r] = ok ? ll : -INFINITY;
        if (l[r] > mx) mx = l[r];
      }
      // (pjm_exp_nonpos: 1 at 0, an exact 0 from -745 down and at -inf, NaN for NaN; mx = +inf cannot come from finite input)
      if (mx > m[c]) { sum[c] *= pjm_exp_nonpos(m[c] - mx, tab); m[c] = mx; }
      if (mx > -INFINITY) {
#pragma unroll
        for (int r = 0; r < 4; ++r) sum[c] += pjm_exp_nonpos(l[r] - mx, tab);
      }
    }
  }
  // the four lanes of a row, in lane order; lanes 0..15 hold the row's record
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    double mm = m[c], ss = sum[c], ll = sl[c];
#pragma unroll
    for (int j = 1; j < 4; ++j) {
      const double m2 = __shfl(m[c], li + 16 * j), s2 = __shfl(sum[c], li + 16 * j), l2 = __shfl(sl[c], li + 16 * j);
      pred_merge(mm, ss, ll, m2, s2, l2);
    }
    const int64_t row = row0 + 16 * c + li;
    if (lk == 0 && row < a.N) {
      double* o = a.rec + ((size_t)blockIdx.y * (size_t)a.N + (size_t)row) * 3;
      o[0] = mm; o[1] = ss; o[2] = ll;
    }
  }
}

__global__ __launch_bounds__(256) void pred_combine_kernel(const double* __restrict__ rec, int64_t N, int splits, int64_t S,
                                                           double* __restrict__ lppd, double* __restrict__ mean) {
  const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (row >= N) return;
  double m = -INFINITY, s = 0.0, l = 0.0;
  for (int i = 0; i < splits; ++i) {
    const double* p = rec + ((size_t)i * (size_t)N + (size_t)row) * 3;
    pred_merge(m, s, l, p[0], p[1], p[2]);
  }
  const double v = m + log(s / (double)S);          // (every ll equal: s = S exactly, log 1 = 0, the value itself)
  lppd[row] = (l != l) ? l : v;
  if (mean) mean[row] = l / (double)S;
}

// ranges of the draws: the caller's count, or enough workgroups to fill the device a few times over while a range keeps
// PRED_MIN_RANGE draws
static int pred_splits(int64_t N, int64_t S, int splits) {
  if (splits > 0) return splits;
  const int cus = cu_count();
  const int64_t tiles = (N + PRED_ROWS - 1) / PRED_ROWS;
  if (tiles < 1) return 1;
  int64_t want = ((int64_t)8 * cus + tiles - 1) / tiles;
  const int64_t most = S / PRED_MIN_RANGE;
  if (want > most) want = most;
  if (want > PRED_MAX_SPLITS) want = PRED_MAX_SPLITS;
  return want < 1 ? 1 : (int)want;
}
static bool pred_shape_ok(int64_t N, int32_t D, int64_t S, int32_t splits) {
  return N >= 0 && N <= ((int64_t)1 << 37) && D >= 1 && D <= PRED_DMAX && S >= 1 && splits >= 0 && splits <= PRED_MAX_SPLITS;
}

extern "C" int64_t bcx_log_predictive_scratch_bytes(int64_t N, int32_t D, int64_t S, int32_t splits) {
  if (!pred_shape_ok(N, D, S, splits)) return -1;
  return (int64_t)pred_splits(N, S, splits) * N * 3 * (int64_t)sizeof(double);
}
extern "C" int bcx_log_predictive(void* stream, int32_t family, const void* Z_dev, int64_t N, int64_t ldz, int32_t D,
                                  const void* Theta_dev, int64_t S, int64_t ldt, int32_t splits, void* lppd_dev, void* mean_dev,
                                  void* work_dev, int64_t work_bytes) {
  if ((family != LAP_LOGISTIC && family != LAP_POISSON) || !pred_shape_ok(N, D, S, splits) || ldt < D || !Theta_dev ||
      (N > 0 && (!Z_dev || !lppd_dev || !work_dev || ldz < D + (family == LAP_POISSON ? 1 : 0) ||
                 work_bytes < bcx_log_predictive_scratch_bytes(N, D, S, splits))))
    return bcx_fail(BCX_ERR_ARG, "bcx_log_predictive", "bad arguments (family 0 logistic / 1 Poisson, 1 <= D <= 32, S >= 1, ldt >= D, 0 <= splits <= "
                                                       "4096, work_dev of bcx_log_predictive_scratch_bytes)");
  if (N == 0) return BCX_OK;
  hipStream_t st = (hipStream_t)stream;
  PredArgs a;
  a.Z = (const double*)Z_dev; a.Th = (const double*)Theta_dev; a.rec = (double*)work_dev;
  if (!(a.tab = proj_tables())) return bcx_fail(BCX_ERR_NOMEM, "bcx_log_predictive", "no device memory for the likelihood tables");
  a.N = N; a.ldz = ldz; a.S = S; a.ldt = ldt; a.D = D; a.splits = pred_splits(N, S, splits);
  const dim3 grid((unsigned)((N + PRED_ROWS - 1) / PRED_ROWS), (unsigned)a.splits);
  if (family == LAP_LOGISTIC) hipLaunchKernelGGL(pred_rows_kernel<LAP_LOGISTIC>, grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL(pred_rows_kernel<LAP_POISSON>, grid, dim3(256), 0, st, a);
  hipLaunchKernelGGL(pred_combine_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, (const double*)work_dev, N, a.splits, S,
                     (double*)lppd_dev, (double*)mean_dev);
  BCX_TRY("bcx_log_predictive", hipGetLastError());
  return BCX_OK;
}
