// hmc.hip -- MCMC on the weighted points, the evaluation a Bayesian coreset is built for (the reference's logistic / Poisson
// experiment, examples/logistic_poisson_regression/main.py:107-127, 205-232, runs Stan on the full data and on every coreset
// with 'w': wts):
//
//  * bcx_log_joint_grad: log_joint(Z, theta, w) = sum_j w_j log p(z_j | theta) - |theta|^2 / 2 - D/2 log 2 pi and its
//    theta-gradient for C parameter vectors at once (model_lr.py:34-39, 59-64; model_poiss.py:40-46, 69-74 -- the Poisson value
//    keeps -log y!).  A workgroup walks its range of rows in tiles of 128: every thread evaluates the per-point function
//    (csrc/lik_point.h, the text the Laplace sampler uses) for one row and four theta columns, the 8 x D outer-product sums of
//    the tile run from LDS with one (column, coordinate) per thread.  Per-workgroup partials in a fixed order, then a
//    fixed-order second level: no floating-point atomics, two runs give the same bits.
//  * bcx_hmc_coreset: Hamiltonian Monte Carlo with one workgroup per chain, the k weighted points resident in LDS for all
//    warm-up and sampling transitions of ONE launch.
//  * bcx_hmc_stream: the same transition for points that do not fit (the full data set): every leapfrog step is one
//    log-joint pass over the resident rows for all chains and one small kernel per chain behind it that adds the partials in
//    a fixed order and runs the SAME transition text (hmc_consume) -- enqueued on the stream, no host synchronisation.
//  * bcx_cmc_advance: the chains of Coreset MCMC -- the coreset kernel's transition from a state carried in global memory, at
//    weights that move between launches, emitting what the weight step reads (cmc_advance_kernel, cmc_centre_kernel).
//
// The chain moves in the whitened variable xi, theta = mu + W^T xi (unit mass matrix; mu, W: the Laplace mode and covariance
// factor by default, W = I: plain HMC).  Transition t of a chain reads D + 3 standard normals (bcx_standard_normal): D momenta,
// two for the accept threshold e = (z1^2 + z2^2) / 2 ~ Exp(1) (accept iff dH <= e), one for the step jitter
// eps_t = eps exp(0.1 z).  A fixed number L of leapfrog steps; the warm-up adapts eps per chain by dual averaging (Hoffman &
// Gelman 2014, Alg. 5: delta 0.8, gamma 0.05, t0 10, kappa 0.75), sampling uses the averaged step.
#include <math.h>
#include <string>
#include "bcx_internal.h"
#include "hmc_core.h"
#include "launch_host.h"

#define HMC_STEP_THREADS 64
#define HMC_DIAG 6
#define LJ_ROWS 128          // rows of a tile
#define LJ_CT 8              // theta columns of a workgroup
#define LJ_MAX_WG 512        // workgroups along the rows (the second level adds that many partials per output)
#define LJ_CCHUNK 256        // theta columns of one launch (bounds the partials)
#define HMC_STREAM_CMAX LJ_CCHUNK

// ---------------------------------------------------------------------------------------------------------------- log joint
struct LjArgs {
  const double* Z;      // N x ldz rows (logistic: y x; Poisson: [x, y])
  const double* w;      // N weights or NULL (ones)
  const double* Th;     // C x ldt parameter vectors
  double* part;         // nwg x C x (D + 1): per-workgroup sums of w g x (D values) and of w log p
  int64_t N, ldz, rows_per_wg;
  int family, D, C, ldt, with_const;
};

__global__ __launch_bounds__(256) void lj_partial_kernel(LjArgs a) {
  __shared__ double sX[LJ_ROWS * HMC_LDW];
  __shared__ double sG[LJ_ROWS * (LJ_CT + 1)];         // w_j g_jc of the tile; at the end the threads' value sums (256 x 4)
  __shared__ double sTh[LJ_CT * HMC_LDW];
  __shared__ double sw[LJ_ROWS], sy[LJ_ROWS], slg[LJ_ROWS];
  const int tid = threadIdx.x, D = a.D;
  const int c0 = blockIdx.y * LJ_CT;
  for (int e = tid; e < LJ_CT * 32; e += 256) {
    const int c = e >> 5, d = e & 31;
    sTh[c * HMC_LDW + d] = (d < D && c0 + c < a.C) ? a.Th[(size_t)(c0 + c) * a.ldt + d] : 0.0;
  }
  const int64_t begin = (int64_t)blockIdx.x * a.rows_per_wg;
  const int64_t end = begin + a.rows_per_wg < a.N ? begin + a.rows_per_wg : a.N;
  const int r = tid & (LJ_ROWS - 1), hq = (tid >> 7) * 4;      // phase A: row r, columns hq .. hq + 3
  const int bc = tid >> 5, bd = tid & 31;                       // phase B: column bc, coordinate bd
  double val[4] = {0.0, 0.0, 0.0, 0.0};
  double acc = 0.0;
  for (int64_t row0 = begin; row0 < end; row0 += LJ_ROWS) {
    __syncthreads();
    for (int e = tid; e < LJ_ROWS * D; e += 256) {
      const int rr = e / D, d = e - rr * D;
      sX[rr * HMC_LDW + d] = row0 + rr < end ? a.Z[(size_t)(row0 + rr) * a.ldz + d] : 0.0;
    }
    if (tid < LJ_ROWS) {
      const bool in = row0 + tid < end;
      const double y = (in && a.family == LAP_POISSON) ? a.Z[(size_t)(row0 + tid) * a.ldz + D] : 0.0;
      sw[tid] = in ? (a.w ? a.w[row0 + tid] : 1.0) : 0.0;      // (a row past the end: x = 0, w = 0 adds an exact zero)
      sy[tid] = y;
      slg[tid] = (a.with_const && a.family == LAP_POISSON) ? lgamma(y + 1.0) : 0.0;
    }
    __syncthreads();
    {
      const double w = sw[r], y = sy[r], lg = slg[r];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        double s = 0.0;
        for (int d = 0; d < D; ++d) s = fma(sX[r * HMC_LDW + d], sTh[(hq + q) * HMC_LDW + d], s);
        double ll, g, h;
        lap_point(a.family, s, y, ll, g, h);
        val[q] += w * (ll - lg);
        sG[r * (LJ_CT + 1) + hq + q] = w * g;
      }
    }
    __syncthreads();
    if (bd < D) {
      for (int rr = 0; rr < LJ_ROWS; ++rr) acc = fma(sG[rr * (LJ_CT + 1) + bc], sX[rr * HMC_LDW + bd], acc);
    }
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < 4; ++q) sG[tid * 4 + q] = val[q];
  __syncthreads();
  double* out = a.part + (size_t)blockIdx.x * a.C * (D + 1);
  if (bd < D && c0 + bc < a.C) out[(size_t)(c0 + bc) * (D + 1) + bd] = acc;
  if (tid < LJ_CT && c0 + tid < a.C) {
    const int base = (tid >> 2) * LJ_ROWS, q = tid & 3;
    double t = 0.0;
    for (int rr = 0; rr < LJ_ROWS; ++rr) t += sG[(base + rr) * 4 + q];
    out[(size_t)(c0 + tid) * (D + 1) + D] = t;
  }
}

// second level: the partials of one output in workgroup order, then the prior (model_lr.py:34-36, 59-61)
__global__ __launch_bounds__(256) void lj_finalize_kernel(const double* __restrict__ part, int nwg, const double* __restrict__ Th, int C,
                                                          int D, int ldt, double* __restrict__ value, double* __restrict__ grad) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)C * (D + 1)) return;
  const int c = (int)(idx / (D + 1)), d = (int)(idx - (int64_t)c * (D + 1));
  double t = 0.0;
  for (int g = 0; g < nwg; ++g) t += part[((size_t)g * C + c) * (D + 1) + d];
  if (d < D) { grad[(size_t)c * ldt + d] = t - Th[(size_t)c * ldt + d]; return; }
  double q = 0.0;
  for (int i = 0; i < D; ++i) q = fma(Th[(size_t)c * ldt + i], Th[(size_t)c * ldt + i], q);
  value[c] = (t - 0.5 * q) - 0.5 * D * 1.8378770664093454835606594728112;    // log 2 pi
}

static int lj_workgroups(int64_t N, int64_t* rows_per_wg) {
  if (N <= 0) { *rows_per_wg = LJ_ROWS; return 0; }
  const int64_t tiles = (N + LJ_ROWS - 1) / LJ_ROWS;
  const int64_t want = tiles < LJ_MAX_WG ? tiles : LJ_MAX_WG;
  const int64_t per = (tiles + want - 1) / want * LJ_ROWS;
  *rows_per_wg = per;
  return (int)((N + per - 1) / per);
}
// one pass over the rows for C <= LJ_CCHUNK columns: part (nwg x C x (D + 1)); returns nwg
static int lj_pass(hipStream_t st, int family, const double* Z, int64_t N, int64_t ldz, int D, const double* w, const double* Th, int C,
                   int ldt, double* part, int with_const) {
  LjArgs a;
  a.Z = Z; a.w = w; a.Th = Th; a.part = part; a.N = N; a.ldz = ldz; a.family = family; a.D = D; a.C = C; a.ldt = ldt;
  a.with_const = with_const;
  const int nwg = lj_workgroups(N, &a.rows_per_wg);
  if (nwg > 0) hipLaunchKernelGGL(lj_partial_kernel, dim3(nwg, (C + LJ_CT - 1) / LJ_CT), dim3(256), 0, st, a);
  return nwg;
}

extern "C" int64_t bcx_log_joint_grad_scratch_bytes(int64_t N, int32_t D, int32_t C) {
  if (N < 0 || D < 1 || D > HMC_DMAX || C < 1) return -1;
  int64_t per;
  const int nwg = lj_workgroups(N, &per);
  return (int64_t)(nwg > 0 ? nwg : 1) * (C < LJ_CCHUNK ? C : LJ_CCHUNK) * (D + 1) * (int64_t)sizeof(double);
}
extern "C" int bcx_log_joint_grad(void* stream, int32_t family, const void* Z_dev, int64_t N, int64_t ldz, int32_t D, const void* w_dev,
                                  const void* Theta_dev, int32_t C, int32_t ldt, void* value_dev, void* grad_dev, void* work_dev) {
  if ((family != LAP_LOGISTIC && family != LAP_POISSON) || N < 0 || D < 1 || D > HMC_DMAX || C < 1 || ldt < D || !Theta_dev || !value_dev ||
      !grad_dev || !work_dev || (N > 0 && (!Z_dev || ldz < D + (family == LAP_POISSON ? 1 : 0))))
    return bcx_fail(BCX_ERR_ARG, "bcx_log_joint_grad", "bad arguments (family 0 logistic / 1 Poisson, D <= 32, ldt >= D, work_dev of "
                                                       "bcx_log_joint_grad_scratch_bytes)");
  hipStream_t st = (hipStream_t)stream;
  for (int c0 = 0; c0 < C; c0 += LJ_CCHUNK) {
    const int cc = C - c0 < LJ_CCHUNK ? C - c0 : LJ_CCHUNK;
    const double* th = (const double*)Theta_dev + (size_t)c0 * ldt;
    const int nwg = lj_pass(st, family, (const double*)Z_dev, N, ldz, D, (const double*)w_dev, th, cc, ldt, (double*)work_dev, 1);
    hipLaunchKernelGGL(lj_finalize_kernel, dim3((unsigned)(((int64_t)cc * (D + 1) + 255) / 256)), dim3(256), 0, st, (const double*)work_dev, nwg,
                       th, cc, (int)D, (int)ldt, (double*)value_dev + c0, (double*)grad_dev + (size_t)c0 * ldt);
  }
  BCX_TRY("bcx_log_joint_grad", hipGetLastError());
  return BCX_OK;
}

// ------------------------------------------------------------------------------------------------------------ the transition
// (HmcPar, HmcChain, HmcLds, the frame, hmc_theta, hmc_reset, the dual averaging: csrc/hmc_core.h)
// start transition t: momentum, threshold, jittered step, the first half kick and drift; leaves th = theta(xp)
static __device__ void hmc_begin(HmcLds& S, const HmcPar& a, int chain, int t) {
  const int tid = threadIdx.x, D = a.D;
  const double* z = a.noise + ((size_t)chain * a.T + t) * (D + 3);
  const double eps_t = S.s.sc[SC_BASE] * exp(0.1 * z[D + 2]);
  const double e = 0.5 * (z[D] * z[D] + z[D + 1] * z[D + 1]);
  const double H0 = hmc_half_sq(z, D) - S.s.sc[SC_LOGP];
  if (tid < D) {
    const double p = z[tid] + (0.5 * eps_t) * S.s.gcur[tid];
    S.s.p[tid] = p;
    S.s.xp[tid] = S.s.xi[tid] + eps_t * p;
  }
  __syncthreads();
  if (tid == 0) { S.s.sc[SC_EPS_T] = eps_t; S.s.sc[SC_H0] = H0; S.s.sc[SC_E] = e; }
  hmc_theta(S, D);
  __syncthreads();
}
// consume one evaluation of the target at th: S.gth = its theta-gradient (prior included), logp its value (constants dropped).
// phase 0: the start state; 1 .. L - 1: a full kick and drift; L: the last half kick, accept / reject, adaptation, outputs and
// the start of the next transition.  Every thread of the workgroup calls it; the state is left synchronised.
static __device__ void hmc_consume(HmcLds& S, const HmcPar& a, int chain, int phase, int t, double logp) {
  const int tid = threadIdx.x, D = a.D;
  double gx = 0.0;
  if (tid < D) for (int c = 0; c < D; ++c) gx = fma(S.W[tid * HMC_LDW + c], S.gth[c], gx);
  if (phase == 0) {
    if (tid < D) { S.s.gcur[tid] = gx; S.s.thcur[tid] = S.s.th[tid]; }
    if (tid == 0) {
      S.s.sc[SC_LOGP] = logp;
      if (!isfinite(logp)) { atomicMax(&a.status[0], 2); atomicMax(&a.status[1], 2); }
    }
    __syncthreads();
    if (a.T > 0) hmc_begin(S, a, chain, 0);
    return;
  }
  const double eps_t = S.s.sc[SC_EPS_T];
  if (phase < a.L) {
    if (tid < D) {
      const double p = S.s.p[tid] + eps_t * gx;
      S.s.p[tid] = p;
      S.s.xp[tid] = S.s.xp[tid] + eps_t * p;
    }
    __syncthreads();
    hmc_theta(S, D);
    __syncthreads();
    return;
  }
  if (tid < D) S.s.p[tid] = S.s.p[tid] + (0.5 * eps_t) * gx;
  __syncthreads();
  const double H1 = hmc_half_sq(S.s.p, D) - logp;
  const double dH = H1 - S.s.sc[SC_H0];
  const bool fin = isfinite(dH);
  const bool acc = fin && dH <= S.s.sc[SC_E];
  double base = S.s.sc[SC_BASE], hbar = S.s.sc[SC_HBAR], lebar = S.s.sc[SC_LEBAR], nacc = S.s.sc[SC_NACC];
  const size_t o = (size_t)chain * a.T + t;
  if (a.props && tid < a.ld) a.props[o * a.ld + tid] = tid < D ? S.s.xp[tid] : 0.0;
  __syncthreads();
  if (acc && tid < D) { S.s.xi[tid] = S.s.xp[tid]; S.s.gcur[tid] = gx; S.s.thcur[tid] = S.s.th[tid]; }
  __syncthreads();
  if (tid < a.ld) {
    a.samples[o * a.ld + tid] = tid < D ? S.s.thcur[tid] : 0.0;
    if (a.xis) a.xis[o * a.ld + tid] = tid < D ? S.s.xi[tid] : 0.0;
  }
  const int life = a.t0 + t;                   // (the transition's index in the chain's life: t but for cmc_advance_kernel)
  if (!(a.fixed_eps > 0.0) && life < a.nwarm) {
    const double alpha = fin ? fmin(1.0, exp(-dH)) : 0.0;
    base = hmc_dual_average(life, a.nwarm, a.eps0, alpha, hbar, lebar);
  }
  if (life >= a.nwarm || a.nwarm >= a.T) nacc += acc ? 1.0 : 0.0;
  if (tid == 0) {
    if (acc) S.s.sc[SC_LOGP] = logp;
    S.s.sc[SC_BASE] = base; S.s.sc[SC_HBAR] = hbar; S.s.sc[SC_LEBAR] = lebar; S.s.sc[SC_NACC] = nacc;
    double* dg = a.diag + o * HMC_DIAG;
    dg[0] = dH; dg[1] = acc ? 1.0 : 0.0; dg[2] = eps_t; dg[3] = base; dg[4] = hbar; dg[5] = lebar;
    if (!fin) { atomicMax(&a.status[0], 1); atomicMax(&a.status[1], 1); }
    if (t + 1 == a.T && a.accept_rate) {       // (cmc_advance_kernel has neither: its caller reads diag)
      const int cnt = a.nwarm >= a.T ? a.T : a.T - a.nwarm;
      a.accept_rate[chain] = nacc / (double)cnt;
      a.eps_final[chain] = base;
    }
  }
  __syncthreads();
  if (t + 1 < a.T) hmc_begin(S, a, chain, t + 1);
}

// ------------------------------------------------------------------------------------------- coreset path: the points in LDS
struct HmcCoresetArgs {
  HmcPar par;
  const double* w;      // k weights or NULL (ones)
  const double* pts;    // k x ldp
  int64_t ldp;
  int family, k;
};

__global__ __launch_bounds__(HMC_THREADS) void hmc_coreset_kernel(HmcCoresetArgs a) {
  extern __shared__ __attribute__((aligned(16))) double hmc_dyn[];
  __shared__ HmcLds S;
  __shared__ double s_part[8 * 32];
  __shared__ double scratch[BCX_SCRATCH];
  const int chain = blockIdx.x, D = a.par.D;
  const HmcPoints P = hmc_load_points(hmc_dyn, a.family, a.k, D, a.w, a.pts, a.ldp);
  hmc_load_frame(S, a.par);
  hmc_reset(S, a.par);
  __syncthreads();
  hmc_theta(S, D);
  __syncthreads();

  auto eval = [&]() -> double { return hmc_eval_points(S, P, D, s_part, scratch); };      // (the target at S.s.th: csrc/hmc_core.h)

  hmc_consume(S, a.par, chain, 0, 0, eval());
  for (int t = 0; t < a.par.T; ++t)
    for (int l = 1; l <= a.par.L; ++l) hmc_consume(S, a.par, chain, l, t, eval());
}

// (the entry points' shared argument check and HmcPar fill, hmc_common_ok and hmc_par: csrc/hmc_core.h)
extern "C" int64_t bcx_hmc_coreset_lds_bytes(int32_t k, int32_t D) {
  if (k < 0 || D < 1 || D > HMC_DMAX) return -1;
  return hmc_points_lds_bytes(k, D);
}
// 1 when one workgroup can hold the k points (D <= 32, the points and three doubles each within the LDS the device gives a
// workgroup, less what the kernel uses itself)
extern "C" int bcx_hmc_coreset_ok(int32_t k, int32_t D) {
  static PerDevice<int64_t> room;
  const int64_t b = bcx_hmc_coreset_lds_bytes(k, D);
  return b >= 0 && b <= lds_room((const void*)hmc_coreset_kernel, room);
}
extern "C" int bcx_hmc_coreset(void* stream, int32_t family, int32_t k, int32_t D, const void* w_dev, const void* pts_dev, int64_t ldp,
                               const void* mu_dev, const void* W_dev, int64_t ldw, int32_t chains, int32_t n_warmup, int32_t n_samples,
                               int32_t leapfrog, double eps0, double fixed_eps, const void* noise_dev, int32_t ld, void* samples_dev,
                               void* xi_dev, void* prop_dev, void* diag_dev, void* accept_dev, void* eps_dev, void* status_dev) {
  if (!hmc_common_ok(family, D, chains, n_warmup, n_samples, eps0, ld, noise_dev, samples_dev, diag_dev, accept_dev, eps_dev, status_dev) ||
      leapfrog < 1 || !bcx_hmc_coreset_ok(k, D) || (W_dev && ldw < D) ||
      (k > 0 && (!pts_dev || ldp < D + (family == LAP_POISSON ? 1 : 0))))
    return bcx_fail(BCX_ERR_ARG, "bcx_hmc_coreset", "bad arguments (family 0 logistic / 1 Poisson, D <= ld <= 32, the points within "
                                                    "bcx_hmc_coreset_ok, at least one transition and leapfrog step, eps0 > 0)");
  HmcCoresetArgs a;
  a.par = hmc_par(D, mu_dev, W_dev, ldw, chains, n_warmup, n_samples, leapfrog, eps0, fixed_eps, noise_dev, ld, samples_dev, xi_dev, prop_dev,
                  diag_dev, accept_dev, eps_dev, status_dev);
  a.w = (const double*)w_dev; a.pts = (const double*)pts_dev; a.ldp = ldp; a.family = family; a.k = k;
  hipStream_t st = (hipStream_t)stream;
  const size_t lds = (size_t)bcx_hmc_coreset_lds_bytes(k, D);
  static PerDevice<size_t> lds_max;
  BCX_TRY("bcx_hmc_coreset", raise_dynamic_lds((const void*)hmc_coreset_kernel, lds, 16 * 1024, lds_max));
  BCX_TRY("bcx_hmc_coreset", hipMemsetAsync(status_dev, 0, sizeof(int), st));
  hipLaunchKernelGGL(hmc_coreset_kernel, dim3(chains), dim3(HMC_THREADS), lds, st, a);
  BCX_TRY("bcx_hmc_coreset", hipGetLastError());
  return BCX_OK;
}

// ------------------------------------------------------------------- Coreset MCMC: the chains of a run whose weights move
// (Chen & Campbell 2024; bayesiancoresets_amd/coreset/coresetmcmc.py)  One launch advances every chain by
// `thin` transitions of the text above at the weights as they are NOW, and emits what the weight step behind it reads:
//   * the chain's HmcChain is loaded from `state` (fresh: hmc_reset) and stored back, so a chain lives across launches;
//   * the target and its gradient at the carried state are evaluated again (phase 0 of hmc_consume): what the previous launch
//     cached belongs to the previous weights;
//   * HmcPar::t0 makes the dual averaging count the transitions of the chain's life, not of the launch;
//   * core[m ldc + chain] = ll(z_m, theta_chain) over the k points and colsum[chain] = sum_r ll(z_rows[r], theta_chain) over
//     the gathered rows of the resident data (rows NULL: all N), at the state after the last transition.
// Nothing waits on another workgroup: the order against the weight step is the launch boundary.  A NaN is kept.
struct CmcArgs {
  HmcPar par;           // T = thin, nwarm = the life-long adapting transitions; noise / samples / xis / props / diag: this launch's block
  const double* w;      // k weights
  const double* pts;    // k x ldp
  HmcChain* state;      // chains
  const double* Z;      // N x ldz: the resident data set
  const int64_t* rows;  // n_rows indices into Z, or NULL (all N rows)
  double* core;         // k x ldc
  double* colsum;       // chains
  int64_t ldp, N, ldz, n_rows, ldc;
  int family, k, fresh;
};

__global__ __launch_bounds__(HMC_THREADS) void cmc_advance_kernel(CmcArgs a) {
  extern __shared__ __attribute__((aligned(16))) double hmc_dyn[];
  __shared__ HmcLds S;
  __shared__ double s_part[8 * 32];
  __shared__ double scratch[BCX_SCRATCH];
  const int tid = threadIdx.x, chain = blockIdx.x, D = a.par.D;
  const HmcPoints P = hmc_load_points(hmc_dyn, a.family, a.k, D, a.w, a.pts, a.ldp);
  hmc_load_frame(S, a.par);
  if (a.fresh) {
    hmc_reset(S, a.par);
  } else {
    double* dst = (double*)&S.s;
    const double* src = (const double*)&a.state[chain];
    for (int e = tid; e < (int)(sizeof(HmcChain) / sizeof(double)); e += HMC_THREADS) dst[e] = src[e];
    if (tid < 32) S.gth[tid] = 0.0;
  }
  __syncthreads();
  if (tid < 32) S.s.xp[tid] = S.s.xi[tid];           // (the stored xp is the last proposal, accepted or not)
  __syncthreads();
  hmc_theta(S, D);
  __syncthreads();

  auto eval = [&]() -> double { return hmc_eval_points(S, P, D, s_part, scratch); };

  hmc_consume(S, a.par, chain, 0, 0, eval());
  for (int t = 0; t < a.par.T; ++t)
    for (int l = 1; l <= a.par.L; ++l) hmc_consume(S, a.par, chain, l, t, eval());
  {
    const double* src = (const double*)&S.s;
    double* dst = (double*)&a.state[chain];
    for (int e = tid; e < (int)(sizeof(HmcChain) / sizeof(double)); e += HMC_THREADS) dst[e] = src[e];
  }
  // what the weight step reads, at thcur
  const int Dp = D + 1;
  for (int j = tid; j < a.k; j += HMC_THREADS) {
    double s = 0.0;
    for (int c = 0; c < D; ++c) s = fma(P.sX[j * Dp + c], S.s.thcur[c], s);
    double ll, g, h;
    lap_point(a.family, s, P.sy[j], ll, g, h);
    a.core[(size_t)j * a.ldc + chain] = ll;
  }
  const int64_t n = a.rows ? a.n_rows : a.N;
  double part[1] = {0.0};
  for (int64_t r = tid; r < n; r += HMC_THREADS) {
    const int64_t i = a.rows ? a.rows[r] : r;
    if ((uint64_t)i >= (uint64_t)a.N) { part[0] += NAN; continue; }      // (an index outside the data is not read: the sum says so)
    const double* row = a.Z + (size_t)i * a.ldz;
    double s = 0.0;
    for (int c = 0; c < D; ++c) s = fma(row[c], S.s.thcur[c], s);
    double ll, g, h;
    lap_point(a.family, s, a.family == LAP_POISSON ? row[D] : 0.0, ll, g, h);
    part[0] += ll;
  }
  block_allsum<1>(part, scratch);                    // (every thread's rows in their order, the lanes, then the waves in theirs)
  if (tid == 0) a.colsum[chain] = part[0];
}

// s <- s - mean(s) over the chains, one workgroup: svi_adam_kernel takes the column sums as they arrive and centres only the points
__global__ __launch_bounds__(256) void cmc_centre_kernel(double* __restrict__ s, int n) {
  __shared__ double scratch[BCX_SCRATCH];
  double part[1] = {0.0};
  for (int c = threadIdx.x; c < n; c += 256) part[0] += s[c];
  block_allsum<1>(part, scratch);
  const double mean = part[0] / (double)n;
  for (int c = threadIdx.x; c < n; c += 256) s[c] -= mean;
}

extern "C" int64_t bcx_cmc_advance_lds_bytes(int32_t k, int32_t D) {
  if (k < 0 || D < 1 || D > HMC_DMAX) return -1;
  return hmc_points_lds_bytes(k, D);
}
extern "C" int bcx_cmc_advance_ok(int32_t k, int32_t D) {
  static PerDevice<int64_t> room;
  const int64_t b = bcx_cmc_advance_lds_bytes(k, D);
  return k >= 1 && k <= 4096 && b >= 0 && b <= lds_room((const void*)cmc_advance_kernel, room);
}
extern "C" int64_t bcx_cmc_state_bytes(int32_t chains) {
  if (chains < 1 || chains > 8192) return -1;
  return (int64_t)chains * (int64_t)sizeof(HmcChain);
}
extern "C" int bcx_cmc_advance(void* stream, int32_t family, int32_t k, int32_t D, const void* w_dev, const void* pts_dev, int64_t ldp,
                               const void* mu_dev, const void* W_dev, int64_t ldw, int32_t chains, int32_t thin, int32_t leapfrog, double eps0,
                               int32_t first_transition, int32_t n_adapt_transitions, int32_t fresh, const void* noise_dev, void* state_dev,
                               const void* Z_dev, int64_t N, int64_t ldz, const void* rows_dev, int64_t n_rows, void* core_dev, int64_t ldc,
                               void* colsum_dev, int32_t ld, void* samples_dev, void* xi_dev, void* prop_dev, void* diag_dev,
                               void* status_dev) {
  const int cols = D + (family == LAP_POISSON ? 1 : 0);
  if ((family != LAP_LOGISTIC && family != LAP_POISSON) || D < 1 || D > HMC_DMAX || chains < 1 || chains > 8192 || thin < 1 || leapfrog < 1 ||
      !(eps0 > 0.0) || first_transition < 0 || (int64_t)first_transition + thin > INT32_MAX || n_adapt_transitions < 0 || ld < D || ld > 32 ||
      !bcx_cmc_advance_ok(k, D) || !w_dev || !pts_dev || ldp < cols || (W_dev && ldw < D) || !noise_dev || !state_dev || N < 1 || !Z_dev ||
      ldz < cols || (rows_dev ? n_rows < 1 : n_rows != 0) || !core_dev || ldc < chains || !colsum_dev || !samples_dev || !diag_dev ||
      !status_dev)
    return bcx_fail(BCX_ERR_ARG, "bcx_cmc_advance", "bad arguments (family 0 logistic / 1 Poisson, D <= ld <= 32, 1 <= k <= 4096 points within "
                                                    "bcx_cmc_advance_ok, at most 8192 chains, ldc >= chains, at least one transition and leapfrog step, eps0 > 0, "
                                                    "n_rows 0 without rows_dev)");
  CmcArgs a;
  a.par = hmc_par(D, mu_dev, W_dev, ldw, chains, n_adapt_transitions, 0, leapfrog, eps0, 0.0, noise_dev, ld, samples_dev, xi_dev, prop_dev,
                  diag_dev, nullptr, nullptr, status_dev);
  a.par.T = thin; a.par.t0 = first_transition;
  a.w = (const double*)w_dev; a.pts = (const double*)pts_dev; a.state = (HmcChain*)state_dev; a.Z = (const double*)Z_dev;
  a.rows = (const int64_t*)rows_dev; a.core = (double*)core_dev; a.colsum = (double*)colsum_dev;
  a.ldp = ldp; a.N = N; a.ldz = ldz; a.n_rows = n_rows; a.ldc = ldc; a.family = family; a.k = k; a.fresh = fresh != 0;
  hipStream_t st = (hipStream_t)stream;
  const size_t lds = (size_t)bcx_cmc_advance_lds_bytes(k, D);
  static PerDevice<size_t> lds_max;
  BCX_TRY("bcx_cmc_advance", raise_dynamic_lds((const void*)cmc_advance_kernel, lds, 16 * 1024, lds_max));
  BCX_TRY("bcx_cmc_advance", hipMemsetAsync(status_dev, 0, sizeof(int), st));
  hipLaunchKernelGGL(cmc_advance_kernel, dim3(chains), dim3(HMC_THREADS), lds, st, a);
  hipLaunchKernelGGL(cmc_centre_kernel, dim3(1), dim3(256), 0, st, (double*)colsum_dev, (int)chains);
  BCX_TRY("bcx_cmc_advance", hipGetLastError());
  return BCX_OK;
}

// ------------------------------------------------------------------------------------- streamed path: the rows in global memory
// One workgroup per chain behind every pass: adds the pass's partials in workgroup order and consumes the evaluation.  `state`
// holds the chains' HmcChain between the kernels, Theta (C x 32) the points the next pass evaluates.
__global__ __launch_bounds__(HMC_STEP_THREADS) void hmc_stream_step_kernel(HmcPar a, HmcChain* state, double* Theta, const double* part,
                                                                           int nwg, int phase, int t) {
  __shared__ HmcLds S;
  __shared__ double s_val;
  const int tid = threadIdx.x, chain = blockIdx.x, D = a.D;
  hmc_load_frame(S, a);
  if (phase == 0) {
    hmc_reset(S, a);
    __syncthreads();
    hmc_theta(S, D);
  } else {
    double* dst = (double*)&S.s;
    const double* src = (const double*)&state[chain];
    for (int e = tid; e < (int)(sizeof(HmcChain) / sizeof(double)); e += HMC_STEP_THREADS) dst[e] = src[e];
  }
  __syncthreads();
  if (tid <= D) {
    double v = 0.0;
    for (int g = 0; g < nwg; ++g) v += part[((size_t)g * a.C + chain) * (D + 1) + tid];
    if (tid < D) S.gth[tid] = v - S.s.th[tid];
    else s_val = v;
  }
  __syncthreads();
  const double logp = s_val - hmc_half_sq(S.s.th, D);
  hmc_consume(S, a, chain, phase, t, logp);
  __syncthreads();
  {
    const double* src = (const double*)&S.s;
    double* dst = (double*)&state[chain];
    for (int e = tid; e < (int)(sizeof(HmcChain) / sizeof(double)); e += HMC_STEP_THREADS) dst[e] = src[e];
  }
  if (tid < 32) Theta[(size_t)chain * 32 + tid] = S.s.th[tid];
}
// Theta = mu for every chain: the point the first pass evaluates
__global__ __launch_bounds__(HMC_STEP_THREADS) void hmc_stream_start_kernel(const double* mu, int D, double* Theta) {
  const int tid = threadIdx.x;
  if (tid < 32) Theta[(size_t)blockIdx.x * 32 + tid] = (tid < D && mu) ? mu[tid] : 0.0;
}

static int64_t hmc_stream_part_offset(int32_t C) {
  return ((int64_t)C * (int64_t)sizeof(HmcChain) + (int64_t)C * 32 * (int64_t)sizeof(double) + 255) / 256 * 256;
}
extern "C" int64_t bcx_hmc_stream_scratch_bytes(int64_t N, int32_t D, int32_t chains) {
  if (N < 0 || D < 1 || D > HMC_DMAX || chains < 1 || chains > HMC_STREAM_CMAX) return -1;
  return hmc_stream_part_offset(chains) + bcx_log_joint_grad_scratch_bytes(N, D, chains);
}
extern "C" int bcx_hmc_stream(void* stream, int32_t family, int64_t N, int32_t D, const void* w_dev, const void* Z_dev, int64_t ldz,
                              const void* mu_dev, const void* W_dev, int64_t ldw, int32_t chains, int32_t n_warmup, int32_t n_samples,
                              int32_t leapfrog, double eps0, double fixed_eps, const void* noise_dev, int32_t ld, void* samples_dev,
                              void* xi_dev, void* prop_dev, void* diag_dev, void* accept_dev, void* eps_dev, void* status_dev, void* work_dev,
                              int64_t work_bytes) {
  if (!hmc_common_ok(family, D, chains, n_warmup, n_samples, eps0, ld, noise_dev, samples_dev, diag_dev, accept_dev, eps_dev, status_dev) ||
      leapfrog < 1 || chains > HMC_STREAM_CMAX || N < 0 || (W_dev && ldw < D) || !work_dev ||
      work_bytes < bcx_hmc_stream_scratch_bytes(N, D, chains) || (N > 0 && (!Z_dev || ldz < D + (family == LAP_POISSON ? 1 : 0))))
    return bcx_fail(BCX_ERR_ARG, "bcx_hmc_stream", "bad arguments (family 0 logistic / 1 Poisson, D <= ld <= 32, at most 256 chains, work_dev of "
                                                   "bcx_hmc_stream_scratch_bytes, at least one transition and leapfrog step, eps0 > 0)");
  const HmcPar p = hmc_par(D, mu_dev, W_dev, ldw, chains, n_warmup, n_samples, leapfrog, eps0, fixed_eps, noise_dev, ld, samples_dev, xi_dev,
                           prop_dev, diag_dev, accept_dev, eps_dev, status_dev);
  hipStream_t st = (hipStream_t)stream;
  HmcChain* state = (HmcChain*)work_dev;
  double* Theta = (double*)((char*)work_dev + (size_t)chains * sizeof(HmcChain));
  double* part = (double*)((char*)work_dev + hmc_stream_part_offset(chains));
  BCX_TRY("bcx_hmc_stream", hipMemsetAsync(status_dev, 0, sizeof(int), st));
  hipLaunchKernelGGL(hmc_stream_start_kernel, dim3(chains), dim3(HMC_STEP_THREADS), 0, st, (const double*)mu_dev, (int)D, Theta);
  auto pass_and_step = [&](int phase, int t) {
    const int nwg = lj_pass(st, family, (const double*)Z_dev, N, ldz, D, (const double*)w_dev, Theta, chains, 32, part, 0);
    hipLaunchKernelGGL(hmc_stream_step_kernel, dim3(chains), dim3(HMC_STEP_THREADS), 0, st, p, state, Theta, (const double*)part, nwg, phase, t);
  };
  pass_and_step(0, 0);
  for (int t = 0; t < p.T; ++t) {
    for (int l = 1; l <= p.L; ++l) pass_and_step(l, t);
    if ((t & 63) == 63) BCX_TRY("bcx_hmc_stream", hipGetLastError());
  }
  BCX_TRY("bcx_hmc_stream", hipGetLastError());
  return BCX_OK;
}
