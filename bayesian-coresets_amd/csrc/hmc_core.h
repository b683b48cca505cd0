// hmc_core.h -- what the samplers on the weighted points share: the chain's frame theta = mu + W^T xi, the target with the k
// points resident in LDS, and the dual averaging of the warm-up.  ONE text for the fixed-length HMC kernels (csrc/hmc.hip) and
// the two NUTS kernels (csrc/nuts.hip, csrc/nuts_stream.hip).  At the end, the host side of the same sharing: the argument check
// their four entry points start with (hmc_common_ok) and the fill of HmcPar (hmc_par).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "dev_util.h"
#include "lik_point.h"

#define HMC_DMAX 32
#define HMC_THREADS 256
#define HMC_LDW 33

struct HmcPar {
  const double* mu;       // D or NULL (zero)
  const double* W;        // D x D, row stride ldw, or NULL (identity): theta = mu + W^T xi
  const double* noise;    // C x T x (D + 3) standard normals
  double* samples;        // C x T x ld: theta after every transition (warm-up included)
  double* xis;            // C x T x ld or NULL: the same states in xi
  double* props;          // C x T x ld or NULL: every transition's proposal in xi
  double* diag;           // C x T x 6: dH, accepted, eps_t, the base step of the next transition, Hbar, log eps-bar
  double* accept_rate;    // C: over the sampling transitions (all of them when there are none)
  double* eps_final;      // C: the step the sampling transitions use
  int* status;            // [0] this launch: 0 ok / 1 a non-finite dH was rejected / 2 non-finite log joint at the start; [1] worst since zeroed
  double eps0, fixed_eps;
  int64_t ldw;
  int D, ld, L, T, nwarm, C;
  int t0;                 // the launch's first transition in the chain's life (0 but for csrc/hmc.hip cmc_advance_kernel: the warm-up counts t0 + t)
};
enum { SC_LOGP = 0, SC_BASE, SC_HBAR, SC_LEBAR, SC_EPS_T, SC_H0, SC_E, SC_NACC, SC_COUNT = 16 };
struct HmcChain {         // one chain's state (LDS; the streamed path keeps a copy in global memory between its kernels)
  double xi[32], xp[32], p[32], gcur[32], thcur[32], th[32], sc[SC_COUNT];
};
struct HmcLds {
  HmcChain s;
  double W[32 * HMC_LDW], mu[32], gth[32];
};

static __device__ __forceinline__ double hmc_half_sq(const double* v, int D) {
  double q = 0.0;
  for (int c = 0; c < D; ++c) q = fma(v[c], v[c], q);
  return 0.5 * q;
}
static __device__ __forceinline__ void hmc_load_frame(HmcLds& S, const HmcPar& a) {
  const int D = a.D;
  for (int e = threadIdx.x; e < 32 * 32; e += blockDim.x) {
    const int i = e >> 5, c = e & 31;
    S.W[i * HMC_LDW + c] = (i < D && c < D) ? (a.W ? a.W[(size_t)i * a.ldw + c] : (i == c ? 1.0 : 0.0)) : 0.0;
  }
  if (threadIdx.x < 32) S.mu[threadIdx.x] = (threadIdx.x < D && a.mu) ? a.mu[threadIdx.x] : 0.0;
}
// th = mu + W^T xp   (callers synchronise around it)
static __device__ __forceinline__ void hmc_theta(HmcLds& S, int D) {
  const int tid = threadIdx.x;
  if (tid < D) {
    double v = S.mu[tid];
    for (int i = 0; i < D; ++i) v = fma(S.W[i * HMC_LDW + tid], S.s.xp[i], v);
    S.s.th[tid] = v;
  }
}
static __device__ __forceinline__ void hmc_reset(HmcLds& S, const HmcPar& a) {
  const int tid = threadIdx.x;
  if (tid < 32) { S.s.xi[tid] = 0.0; S.s.xp[tid] = 0.0; S.s.p[tid] = 0.0; S.s.gcur[tid] = 0.0; S.s.thcur[tid] = 0.0; S.s.th[tid] = 0.0; S.gth[tid] = 0.0; }
  if (tid < SC_COUNT) S.s.sc[tid] = tid == SC_BASE ? (a.fixed_eps > 0.0 ? a.fixed_eps : a.eps0) : 0.0;
}

// dual averaging, iteration m = t + 1 after a transition with accept statistic alpha (Hoffman & Gelman 2014, Alg. 5: delta 0.8,
// gamma 0.05, t0 10, kappa 0.75, mu = log(10 eps0)): updates Hbar and log eps-bar, returns the next base step (eps-bar after the
// last warm-up iteration)
static __device__ __forceinline__ double hmc_dual_average(int t, int nwarm, double eps0, double alpha, double& hbar, double& lebar) {
  const double m = (double)(t + 1);
  const double eta = 1.0 / (m + 10.0);
  hbar = (1.0 - eta) * hbar + eta * (0.8 - alpha);
  const double loge = log(10.0 * eps0) - (sqrt(m) / 0.05) * hbar;
  const double mk = pow(m, -0.75);
  lebar = mk * loge + (1.0 - mk) * lebar;
  return (t + 1 == nwarm) ? exp(lebar) : exp(loge);
}

// ---------------------------------------------------------------------------------------------- the k points resident in LDS
// bytes of dynamic LDS for k points of D parameters: rows of D + 1 doubles, weights, responses, w_j g_j
static inline int64_t hmc_points_lds_bytes(int32_t k, int32_t D) {
  return ((int64_t)k * (D + 1) + 3 * (int64_t)k) * (int64_t)sizeof(double);
}
struct HmcPoints {
  double* sX;             // k x (D + 1) features (rows of D + 1 doubles: consecutive points on different banks)
  double* sw;             // k weights
  double* sy;             // k responses (Poisson)
  double* sg;             // k: w_j g_j
  int family, k;
};
// lay the points out in `dyn` (hmc_points_lds_bytes) and fill them; w NULL: ones.  Callers synchronise behind it.
static __device__ __forceinline__ HmcPoints hmc_load_points(double* dyn, int family, int k, int D, const double* w, const double* pts,
                                                            int64_t ldp) {
  const int tid = threadIdx.x, Dp = D + 1;
  HmcPoints P;
  P.sX = dyn;
  P.sw = P.sX + (size_t)k * Dp;
  P.sy = P.sw + k;
  P.sg = P.sy + k;
  P.family = family; P.k = k;
  for (int e = tid; e < k * D; e += HMC_THREADS) { const int j = e / D, c = e - j * D; P.sX[j * Dp + c] = pts[(size_t)j * ldp + c]; }
  for (int j = tid; j < k; j += HMC_THREADS) {
    P.sw[j] = w ? w[j] : 1.0;
    P.sy[j] = family == LAP_POISSON ? pts[(size_t)j * ldp + D] : 0.0;
  }
  return P;
}
// the target at S.s.th: returns sum_j w_j log p_j - |theta|^2 / 2 and leaves its theta-gradient in S.gth.  Every thread of the
// HMC_THREADS calls it and receives the same value; the state is left synchronised.  s_part: 8 x 32 doubles, scratch: BCX_SCRATCH.
static __device__ __forceinline__ double hmc_eval_points(HmcLds& S, const HmcPoints& P, int D, double* s_part, double* scratch) {
  const int tid = threadIdx.x, k = P.k, Dp = D + 1;
  double part[1] = {0.0};
  for (int j = tid; j < k; j += HMC_THREADS) {
    double s = 0.0;
    for (int c = 0; c < D; ++c) s = fma(P.sX[j * Dp + c], S.s.th[c], s);
    double ll, g, h;
    lap_point(P.family, s, P.sy[j], ll, g, h);
    part[0] += P.sw[j] * ll;
    P.sg[j] = P.sw[j] * g;
  }
  block_allsum<1>(part, scratch);
  {
    const int c = tid & 31, q = tid >> 5;             // eight interleaved slices of the points per coordinate
    double t = 0.0;
    if (c < D) for (int j = q; j < k; j += 8) t = fma(P.sg[j], P.sX[j * Dp + c], t);
    s_part[q * 32 + c] = t;
  }
  __syncthreads();
  if (tid < D) {
    double t = s_part[tid];
    for (int q = 1; q < 8; ++q) t += s_part[q * 32 + tid];
    S.gth[tid] = t - S.s.th[tid];
  }
  __syncthreads();
  return part[0] - hmc_half_sq(S.s.th, D);
}

// ------------------------------------------------------------------------------------ host side: what every entry point checks
// The arguments bcx_hmc_coreset, bcx_hmc_stream, bcx_nuts_coreset and bcx_nuts_stream have in common; each adds its own next to
// the call (the leapfrog count or the tree depth, where the points are, the scratch).  T = n_warmup + n_samples is formed in 64
// bits: HmcPar::T is an int.
static inline bool hmc_common_ok(int32_t family, int32_t D, int32_t chains, int32_t n_warmup, int32_t n_samples, double eps0, int32_t ld,
                                 const void* noise, const void* samples, const void* diag, const void* acc, const void* eps,
                                 const void* status) {
  const int64_t T = (int64_t)n_warmup + n_samples;
  return (family == LAP_LOGISTIC || family == LAP_POISSON) && D >= 1 && D <= HMC_DMAX && chains >= 1 && n_warmup >= 0 && n_samples >= 0 &&
         T >= 1 && T <= INT32_MAX && eps0 > 0.0 && ld >= D && ld <= 32 && noise && samples && diag && acc && eps && status;
}
// (leapfrog: the fixed number of steps; NUTS passes 0)
static inline HmcPar hmc_par(int32_t D, const void* mu, const void* W, int64_t ldw, int32_t chains, int32_t n_warmup, int32_t n_samples,
                             int32_t leapfrog, double eps0, double fixed_eps, const void* noise, int32_t ld, void* samples, void* xi,
                             void* prop, void* diag, void* acc, void* eps, void* status) {
  HmcPar p;
  p.mu = (const double*)mu; p.W = (const double*)W; p.noise = (const double*)noise; p.samples = (double*)samples; p.xis = (double*)xi;
  p.props = (double*)prop; p.diag = (double*)diag; p.accept_rate = (double*)acc; p.eps_final = (double*)eps; p.status = (int*)status;
  p.eps0 = eps0; p.fixed_eps = fixed_eps; p.ldw = ldw; p.D = D; p.ld = ld; p.L = leapfrog; p.T = n_warmup + n_samples; p.nwarm = n_warmup;
  p.C = chains; p.t0 = 0;
  return p;
}
