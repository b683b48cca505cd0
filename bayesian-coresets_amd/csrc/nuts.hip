// nuts.hip -- the No-U-Turn sampler (Hoffman & Gelman 2014) on the weighted points, for the case csrc/hmc.hip runs as one
// launch: one workgroup per chain, the k points resident in LDS for all warm-up and sampling transitions.  The reference's
// logistic / Poisson experiment scores a coreset with Stan, whose sampler is NUTS; the fixed leapfrog count of bcx_hmc_coreset is
// the one knob this removes.
//
// The chain moves in xi, theta = mu + W^T xi, unit mass matrix, the target, frame and dual averaging of csrc/hmc_core.h.  With
// J = max_depth, transition t of a chain reads R = D + 3 J + 2 (2^J - 1) standard normals: D momenta; per doubling j the
// direction (z >= 0: forward) and two for the threshold e_j = (a^2 + b^2) / 2 ~ Exp(1); per leaf slot 2^j - 1 + i two for
// e_leaf.  Doubling j integrates 2^j leapfrog steps of v eps from the right (v = +1) or left endpoint, one target evaluation per
// leaf.  Leaf i: delta = H0 - H_leaf; the accept statistic gains min(1, exp delta); not (finite and delta > -1000) is a
// divergence; logS = logaddexp(logS, delta) and the leaf becomes the doubling's proposal iff logS - delta <= e_leaf; every balanced
// span of leaves that closes at i (one per trailing one bit of i) is tested for a U-turn against the endpoint of its first leaf,
// which even leaf a left at checkpoint slot popcount(a) -- at most J slots.  A divergence or a turn discards the doubling and
// stops the tree.  A completed doubling replaces the tree's proposal iff logW - logS <= e_j (biased progressive sampling), then
// the tree stops if its own endpoints turn.  The selected state carries its log target, gradient and theta.
//
// Every branch is taken by the whole workgroup: each thread computes the decision from the same LDS values (or from scalars
// every thread derived identically from them), and all loops are bounded by integers -- at most 2^J - 1 leaves per transition.
//
// The kernel is a template on whether it learns a metric in the warm-up (bcx_nuts_adapt; csrc/nuts_adapt.h).  A
// metric is a frame: at the end of each warm-up window the chain's S.W, coordinate and carried gradient are re-expressed, the
// dual averaging starts a new segment, and the transition itself is the text below either way.  The instantiation that does not
// adapt carries none of it.
//
// The chain is one device function, nuts_chain, that two kernels call: nuts_coreset_kernel (one posterior, a workgroup per chain)
// and nuts_batch_kernel (bcx_nuts_batch, DESIGN.md 4.18: P posteriors of one family, D, depth and transition counts, P x C
// workgroups, a table in device memory from dispatch slot to problem).
#include <algorithm>
#include <string>
#include <type_traits>
#include <vector>
#include "bcx_internal.h"
#include "hmc_core.h"
#include "nuts_core.h"
#include "nuts_adapt.h"
#include "launch_host.h"

struct NutsArgs {
  HmcPar par;           // (noise: C x T rows of stride noise_ld; L unused; diag: C x T x 8)
  const double* w;      // k weights or NULL (ones)
  const double* pts;    // k x ldp
  int64_t ldp, noise_ld;
  int family, k, J;
};
struct NutsAdaptArgs {
  NutsArgs nuts;
  double* frames;       // C x max(nwin, 1) x D x D: L after each window
  double* metric_out;   // C x D x D: the final L
  int metric, nwin;
  int win[2 * NUTS_ADAPT_WINDOWS];   // start, end of every window
};
static __device__ __forceinline__ const NutsArgs& nuts_args(const NutsArgs& a) { return a; }
static __device__ __forceinline__ const NutsArgs& nuts_args(const NutsAdaptArgs& a) { return a.nuts; }
// (NutsTree, nuts_logaddexp, nuts_threshold and the limits: csrc/nuts_core.h, shared with csrc/nuts_stream.hip)
// One chain, start to end: what a workgroup of either kernel below runs.  `a` is the NutsArgs view the chain works from -- that of
// `args`, or a copy with one problem's points, frame and status put in (nuts_batch_kernel) -- and `chain` the chain's index into
// the noise and every output; `args` itself is read for the metric's fields only.
template <bool ADAPT>
static __device__ __forceinline__ void nuts_chain(const std::conditional_t<ADAPT, NutsAdaptArgs, NutsArgs>& args, const NutsArgs& a,
                                                  const size_t chain) {
  extern __shared__ __attribute__((aligned(16))) double nuts_dyn[];
  __shared__ HmcLds S;
  __shared__ NutsTree Tr;
  __shared__ double s_part[8 * 32];
  __shared__ double scratch[BCX_SCRATCH];
  const int tid = threadIdx.x;
  const int D = a.par.D, J = a.J, T = a.par.T, nwarm = a.par.nwarm, ld = a.par.ld;
  const HmcPoints P = hmc_load_points(nuts_dyn, a.family, a.k, D, a.w, a.pts, a.ldp);
  hmc_load_frame(S, a.par);
  hmc_reset(S, a.par);
  __syncthreads();
  hmc_theta(S, D);
  __syncthreads();

  // the start state xi = 0: its log target, xi-gradient and theta
  double logp_cur = hmc_eval_points(S, P, D, s_part, scratch);
  if (tid < D) {
    double gx = 0.0;
    for (int c = 0; c < D; ++c) gx = fma(S.W[tid * HMC_LDW + c], S.gth[c], gx);
    S.s.gcur[tid] = gx;
    S.s.thcur[tid] = S.s.th[tid];
  }
  if (tid == 0 && !isfinite(logp_cur)) { atomicMax(&a.par.status[0], 2); atomicMax(&a.par.status[1], 2); }
  __syncthreads();

  const bool adapt = !(a.par.fixed_eps > 0.0);
  double base = adapt ? a.par.eps0 : a.par.fixed_eps, hbar = 0.0, lebar = 0.0, acc_sum = 0.0;
  // ADAPT: the window being filled (wi, its draws so far wn) and the dual-averaging segment [seg0, seg1) with its start step
  // (without it A is a byte nobody touches, which the compiler drops: the static LDS stays 20 864 B)
  __shared__ std::conditional_t<ADAPT, NutsAdaptLds, char> A;
  int wi = 0, wn = 0, seg0 = 0, seg1 = nwarm;
  double seg_eps = a.par.eps0;
  if constexpr (ADAPT) {
    nuts_adapt_init(A, S);
    if (args.nwin > 0) seg1 = args.win[1];
    __syncthreads();
  }
  for (int t = 0; t < T; ++t) {
    const double* z = a.par.noise + (chain * T + t) * a.noise_ld;
    const double eps = base;
    const double H0 = hmc_half_sq(z, D) - logp_cur;
    if (tid < D) {
      const double p0 = z[tid], x0 = S.s.xi[tid], g0 = S.s.gcur[tid];
      Tr.xl[tid] = x0; Tr.pl[tid] = p0; Tr.gl[tid] = g0;
      Tr.xr[tid] = x0; Tr.pr[tid] = p0; Tr.gr[tid] = g0;
    }
    double logW = 0.0, asum = 0.0, dsel = 0.0;
    int nleaf = 0, depth = 0;
    bool divergent = false;
    __syncthreads();
    for (int j = 0; j < J; ++j) {
      const bool fwd = z[D + 3 * j] >= 0.0;
      const double v = fwd ? 1.0 : -1.0;
      const double ej = nuts_threshold(z + D + 3 * j + 1);
      if (tid < D) {
        S.s.xp[tid] = fwd ? Tr.xr[tid] : Tr.xl[tid];
        S.s.p[tid] = fwd ? Tr.pr[tid] : Tr.pl[tid];
        Tr.gm[tid] = fwd ? Tr.gr[tid] : Tr.gl[tid];
      }
      __syncthreads();
      const double he = v * (0.5 * eps), ve = v * eps;
      const double* zl = z + D + 3 * J + 2 * ((1 << j) - 1);
      double logS = 0.0, logp_s = 0.0, h_s = 0.0;
      bool ok = true;
      for (int i = 0; i < (1 << j); ++i) {
        // one leapfrog step of v eps from the moving end
        if (tid < D) {
          const double ph = S.s.p[tid] + he * Tr.gm[tid];
          S.s.p[tid] = ph;
          S.s.xp[tid] = S.s.xp[tid] + ve * ph;
        }
        __syncthreads();
        hmc_theta(S, D);
        __syncthreads();
        const double logp = hmc_eval_points(S, P, D, s_part, scratch);
        if (tid < D) {
          double gx = 0.0;
          for (int c = 0; c < D; ++c) gx = fma(S.W[tid * HMC_LDW + c], S.gth[c], gx);
          Tr.gm[tid] = gx;
          S.s.p[tid] = S.s.p[tid] + he * gx;
        }
        __syncthreads();
        const double Hl = hmc_half_sq(S.s.p, D) - logp;
        const double delta = H0 - Hl;
        const bool fin = isfinite(delta);
        asum += fin ? fmin(1.0, exp(delta)) : 0.0;
        ++nleaf;
        if (!fin && tid == 0) { atomicMax(&a.par.status[0], 1); atomicMax(&a.par.status[1], 1); }
        if (!(fin && delta > NUTS_DIVERGENT)) { divergent = true; ok = false; break; }
        bool take = true;
        if (i == 0) {
          logS = delta;
        } else {
          logS = nuts_logaddexp(logS, delta);
          take = logS - delta <= nuts_threshold(zl + 2 * i);
        }
        if (take) {
          if (tid < D) { Tr.xs[tid] = S.s.xp[tid]; Tr.gs[tid] = Tr.gm[tid]; Tr.ths[tid] = S.s.th[tid]; }
          logp_s = logp; h_s = Hl;
        }
        if (i & 1) {
          // the balanced spans that close here: leaves i - 2^m + 1 .. i for every trailing one bit of i
          for (int m = 1; m <= j && ((i >> (m - 1)) & 1); ++m) {
            const int slot = __popc((unsigned)(i - (1 << m) + 1));
            double da = 0.0, db = 0.0;
            for (int c = 0; c < D; ++c) {
              const double d = v * (S.s.xp[c] - Tr.ckx[slot][c]);
              da = fma(d, Tr.ckp[slot][c], da);
              db = fma(d, S.s.p[c], db);
            }
            if (da < 0.0 || db < 0.0) { ok = false; break; }
          }
        } else if (tid < D) {
          const int slot = __popc((unsigned)i);
          Tr.ckx[slot][tid] = S.s.xp[tid];
          Tr.ckp[slot][tid] = S.s.p[tid];
        }
        __syncthreads();
        if (!ok) break;
      }
      if (!ok) break;                       // a divergence or a turn inside the doubling: it is discarded, the tree stops
      if (logW - logS <= ej) {
        if (tid < D) { S.s.xi[tid] = Tr.xs[tid]; S.s.gcur[tid] = Tr.gs[tid]; S.s.thcur[tid] = Tr.ths[tid]; }
        logp_cur = logp_s;
        dsel = h_s - H0;
      }
      logW = nuts_logaddexp(logW, logS);
      if (tid < D) {
        if (fwd) { Tr.xr[tid] = S.s.xp[tid]; Tr.pr[tid] = S.s.p[tid]; Tr.gr[tid] = Tr.gm[tid]; }
        else { Tr.xl[tid] = S.s.xp[tid]; Tr.pl[tid] = S.s.p[tid]; Tr.gl[tid] = Tr.gm[tid]; }
      }
      depth = j + 1;
      __syncthreads();
      double da = 0.0, db = 0.0;
      for (int c = 0; c < D; ++c) {
        const double d = Tr.xr[c] - Tr.xl[c];
        da = fma(d, Tr.pl[c], da);
        db = fma(d, Tr.pr[c], db);
      }
      if (da < 0.0 || db < 0.0) break;
    }
    __syncthreads();
    // the new state is the selected one; outputs, adaptation
    const size_t o = chain * T + t;
    if (tid < ld) {
      a.par.samples[o * ld + tid] = tid < D ? S.s.thcur[tid] : 0.0;
      if (a.par.xis) a.par.xis[o * ld + tid] = tid < D ? S.s.xi[tid] : 0.0;
      if (a.par.props) a.par.props[o * ld + tid] = tid < D ? S.s.xi[tid] : 0.0;
    }
    const double alpha = asum / (double)nleaf;
    if constexpr (ADAPT) {
      if (adapt && t < nwarm) base = hmc_dual_average(t - seg0, seg1 - seg0, seg_eps, alpha, hbar, lebar);
    } else {
      if (adapt && t < nwarm) base = hmc_dual_average(t, nwarm, a.par.eps0, alpha, hbar, lebar);
    }
    if (t >= nwarm || nwarm >= T) acc_sum += alpha;
    if (tid == 0) {
      double* dg = a.par.diag + o * NUTS_DIAG;
      dg[0] = alpha; dg[1] = (double)depth; dg[2] = (double)nleaf; dg[3] = base; dg[4] = hbar; dg[5] = lebar;
      dg[6] = divergent ? 1.0 : 0.0; dg[7] = dsel;
      if (t + 1 == T) {
        const int cnt = nwarm >= T ? T : T - nwarm;
        a.par.accept_rate[chain] = acc_sum / (double)cnt;
        a.par.eps_final[chain] = base;
      }
    }
    __syncthreads();
    if constexpr (ADAPT) {
      if (wi < args.nwin && t >= args.win[2 * wi]) {
        const int wend = args.win[2 * wi + 1];
        nuts_adapt_accumulate(A, S, D, ++wn);
        if (t + 1 == wend) {
          // the window's metric becomes the frame; the state in it, its log target and gradient (theta moves by rounding only)
          nuts_adapt_window_end(A, S, D, wn, args.metric);
          if (tid < D) S.s.xp[tid] = S.s.xi[tid];
          __syncthreads();
          hmc_theta(S, D);
          __syncthreads();
          logp_cur = hmc_eval_points(S, P, D, s_part, scratch);
          if (tid < D) {
            double gx = 0.0;
            for (int c = 0; c < D; ++c) gx = fma(S.W[tid * HMC_LDW + c], S.gth[c], gx);
            S.s.gcur[tid] = gx;
            S.s.thcur[tid] = S.s.th[tid];
          }
          if (a.par.props && tid < ld) a.par.props[o * ld + tid] = tid < D ? S.s.xi[tid] : 0.0;    // (the state in the new frame)
          double* fr = args.frames + (chain * args.nwin + wi) * D * D;
          for (int e = tid; e < D * D; e += HMC_THREADS) { const int i = e / D; fr[e] = A.L[i * HMC_LDW + (e - i * D)]; }
          hbar = 0.0; lebar = 0.0; seg_eps = base; seg0 = wend;
          ++wi; wn = 0;
          seg1 = wi < args.nwin ? args.win[2 * wi + 1] : nwarm;
          __syncthreads();
        }
      }
    }
  }
  if constexpr (ADAPT) {
    double* mo = args.metric_out + chain * D * D;
    for (int e = tid; e < D * D; e += HMC_THREADS) { const int i = e / D; mo[e] = A.L[i * HMC_LDW + (e - i * D)]; }
    if (args.nwin == 0) {                   // (no window: the one frame slot holds the identity)
      double* fr = args.frames + chain * D * D;
      for (int e = tid; e < D * D; e += HMC_THREADS) { const int i = e / D; fr[e] = A.L[i * HMC_LDW + (e - i * D)]; }
    }
  }
}
template <bool ADAPT>
__global__ __launch_bounds__(HMC_THREADS) void nuts_coreset_kernel(std::conditional_t<ADAPT, NutsAdaptArgs, NutsArgs> args) {
  nuts_chain<ADAPT>(args, nuts_args(args), blockIdx.x);
}
// P posteriors in one launch (bcx_nuts_batch): P x C workgroups, workgroup b chain b % C of dispatch slot b / C.
// `table` maps the slot to its problem: the record read once, here, into workgroup-uniform values -- the points, the frame, the
// problem's place p in the caller's order, which is where its noise, outputs (chain p C + c) and two status words are.  The
// launch's dynamic LDS is that of the largest problem; a workgroup lays out its own k points in it.
template <bool ADAPT>
__global__ __launch_bounds__(HMC_THREADS) void nuts_batch_kernel(std::conditional_t<ADAPT, NutsAdaptArgs, NutsArgs> args,
                                                                 const bcx_nuts_problem* __restrict__ table) {
  NutsArgs a = nuts_args(args);
  const int C = a.par.C, slot = (int)blockIdx.x / C;
  const bcx_nuts_problem q = table[slot];
  a.w = (const double*)q.w_dev; a.pts = (const double*)q.pts_dev; a.ldp = q.ldp; a.k = q.k;
  a.par.mu = (const double*)q.mu_dev; a.par.W = (const double*)q.W_dev; a.par.ldw = q.ldw;
  a.par.status += 2 * (size_t)q.index;
  nuts_chain<ADAPT>(args, a, (size_t)q.index * C + ((int)blockIdx.x - slot * C));
}

extern "C" int64_t bcx_nuts_coreset_lds_bytes(int32_t k, int32_t D) {
  if (k < 0 || D < 1 || D > HMC_DMAX) return -1;
  return hmc_points_lds_bytes(k, D);
}
// 1 when one workgroup can hold the k points: within the LDS the device gives a workgroup, less this kernel's static use
extern "C" int bcx_nuts_coreset_ok(int32_t k, int32_t D) {
  static PerDevice<int64_t> room;
  const int64_t b = bcx_nuts_coreset_lds_bytes(k, D);
  return b >= 0 && b <= lds_room((const void*)nuts_coreset_kernel<false>, room);
}
extern "C" int bcx_nuts_coreset(void* stream, int32_t family, int32_t k, int32_t D, const void* w_dev, const void* pts_dev, int64_t ldp,
                                const void* mu_dev, const void* W_dev, int64_t ldw, int32_t chains, int32_t n_warmup, int32_t n_samples,
                                int32_t max_depth, double eps0, double fixed_eps, const void* noise_dev, int64_t noise_ld, int32_t ld,
                                void* samples_dev, void* xi_dev, void* prop_dev, void* diag_dev, void* accept_dev, void* eps_dev,
                                void* status_dev) {
  if (!hmc_common_ok(family, D, chains, n_warmup, n_samples, eps0, ld, noise_dev, samples_dev, diag_dev, accept_dev, eps_dev, status_dev) ||
      max_depth < 1 || max_depth > NUTS_JMAX || noise_ld < nuts_noise_row(D, max_depth) || !bcx_nuts_coreset_ok(k, D) ||
      (W_dev && ldw < D) || (k > 0 && (!pts_dev || ldp < D + (family == LAP_POISSON ? 1 : 0))))
    return bcx_fail(BCX_ERR_ARG, "bcx_nuts_coreset", "bad arguments (family 0 logistic / 1 Poisson, D <= ld <= 32, the points within "
                                                     "bcx_nuts_coreset_ok, at least one transition, max_depth 1 .. 10, noise_ld >= D + 3 max_depth + "
                                                     "2 (2^max_depth - 1), eps0 > 0)");
  NutsArgs a;
  a.par = hmc_par(D, mu_dev, W_dev, ldw, chains, n_warmup, n_samples, 0, eps0, fixed_eps, noise_dev, ld, samples_dev, xi_dev, prop_dev,
                  diag_dev, accept_dev, eps_dev, status_dev);
  a.w = (const double*)w_dev; a.pts = (const double*)pts_dev; a.ldp = ldp; a.noise_ld = noise_ld; a.family = family; a.k = k; a.J = max_depth;
  hipStream_t st = (hipStream_t)stream;
  const size_t lds = (size_t)bcx_nuts_coreset_lds_bytes(k, D);
  static PerDevice<size_t> lds_max;
  BCX_TRY("bcx_nuts_coreset", raise_dynamic_lds((const void*)nuts_coreset_kernel<false>, lds, 16 * 1024, lds_max));
  BCX_TRY("bcx_nuts_coreset", hipMemsetAsync(status_dev, 0, sizeof(int), st));
  hipLaunchKernelGGL(nuts_coreset_kernel<false>, dim3(chains), dim3(HMC_THREADS), lds, st, a);
  BCX_TRY("bcx_nuts_coreset", hipGetLastError());
  return BCX_OK;
}

// ------------------------------------------------------------------------------- the same with a metric learned in the warm-up
extern "C" int32_t bcx_nuts_adapt_schedule(int32_t n_warmup, int32_t* bounds, int32_t cap) {
  return nuts_adapt_schedule(n_warmup, bounds, cap < 0 ? 0 : cap);
}
// 1 when one workgroup can hold the k points next to the adapting instantiation's static LDS (the accumulators, L and W0)
extern "C" int bcx_nuts_adapt_ok(int32_t k, int32_t D) {
  static PerDevice<int64_t> room;
  const int64_t b = bcx_nuts_coreset_lds_bytes(k, D);
  return b >= 0 && b <= lds_room((const void*)nuts_coreset_kernel<true>, room);
}
extern "C" int bcx_nuts_adapt(void* stream, int32_t family, int32_t k, int32_t D, const void* w_dev, const void* pts_dev, int64_t ldp,
                              const void* mu_dev, const void* W_dev, int64_t ldw, int32_t chains, int32_t n_warmup, int32_t n_samples,
                              int32_t max_depth, double eps0, double fixed_eps, const void* noise_dev, int64_t noise_ld, int32_t ld,
                              void* samples_dev, void* xi_dev, void* prop_dev, void* diag_dev, void* accept_dev, void* eps_dev,
                              void* status_dev, int32_t metric, void* frames_dev, void* metric_dev) {
  if (!hmc_common_ok(family, D, chains, n_warmup, n_samples, eps0, ld, noise_dev, samples_dev, diag_dev, accept_dev, eps_dev, status_dev) ||
      max_depth < 1 || max_depth > NUTS_JMAX || noise_ld < nuts_noise_row(D, max_depth) || !bcx_nuts_adapt_ok(k, D) ||
      (W_dev && ldw < D) || (k > 0 && (!pts_dev || ldp < D + (family == LAP_POISSON ? 1 : 0))) ||
      (metric != NUTS_METRIC_DIAG && metric != NUTS_METRIC_DENSE) || fixed_eps > 0.0 || !frames_dev || !metric_dev)
    return bcx_fail(BCX_ERR_ARG, "bcx_nuts_adapt", "bad arguments (those of bcx_nuts_coreset with the points within bcx_nuts_adapt_ok; metric 1 "
                                                   "diag / 2 dense; no fixed_eps with a metric; frames_dev and metric_dev)");
  NutsAdaptArgs g;
  NutsArgs& a = g.nuts;
  a.par = hmc_par(D, mu_dev, W_dev, ldw, chains, n_warmup, n_samples, 0, eps0, fixed_eps, noise_dev, ld, samples_dev, xi_dev, prop_dev,
                  diag_dev, accept_dev, eps_dev, status_dev);
  a.w = (const double*)w_dev; a.pts = (const double*)pts_dev; a.ldp = ldp; a.noise_ld = noise_ld; a.family = family; a.k = k; a.J = max_depth;
  g.frames = (double*)frames_dev; g.metric_out = (double*)metric_dev; g.metric = metric;
  for (int i = 0; i < 2 * NUTS_ADAPT_WINDOWS; ++i) g.win[i] = 0;
  g.nwin = nuts_adapt_schedule(n_warmup, g.win, NUTS_ADAPT_WINDOWS);
  if (g.nwin > NUTS_ADAPT_WINDOWS) return bcx_fail(BCX_ERR_ARG, "bcx_nuts_adapt", "more than 32 warm-up windows");
  hipStream_t st = (hipStream_t)stream;
  const size_t lds = (size_t)bcx_nuts_coreset_lds_bytes(k, D);
  static PerDevice<size_t> lds_max;
  BCX_TRY("bcx_nuts_adapt", raise_dynamic_lds((const void*)nuts_coreset_kernel<true>, lds, 0, lds_max));   // (its static LDS is past 48 KiB)
  BCX_TRY("bcx_nuts_adapt", hipMemsetAsync(status_dev, 0, sizeof(int), st));
  hipLaunchKernelGGL(nuts_coreset_kernel<true>, dim3(chains), dim3(HMC_THREADS), lds, st, g);
  BCX_TRY("bcx_nuts_adapt", hipGetLastError());
  return BCX_OK;
}

// ------------------------------------------------------------------------------------------ many posteriors in one launch
extern "C" int64_t bcx_nuts_batch_table_bytes(int32_t P) {
  return P < 1 ? -1 : (int64_t)P * (int64_t)sizeof(bcx_nuts_problem);
}
// room for dynamic LDS next to the batch kernel's own static use (the same text as the single kernel's, asked of the kernel launched)
template <bool ADAPT>
static bool nuts_batch_fits(int64_t bytes) {
  static PerDevice<int64_t> room;
  return bytes >= 0 && bytes <= lds_room((const void*)nuts_batch_kernel<ADAPT>, room);
}
template <bool ADAPT, class Args>
static int nuts_batch_launch(const Args& g, const bcx_nuts_problem* table, int32_t P, int32_t chains, size_t lds, size_t threshold,
                             hipStream_t st) {
  static PerDevice<size_t> lds_max;
  BCX_TRY("bcx_nuts_batch", raise_dynamic_lds((const void*)nuts_batch_kernel<ADAPT>, lds, threshold, lds_max));
  hipLaunchKernelGGL(nuts_batch_kernel<ADAPT>, dim3((unsigned)P * (unsigned)chains), dim3(HMC_THREADS), lds, st, g, table);
  BCX_TRY("bcx_nuts_batch", hipGetLastError());
  return BCX_OK;
}
extern "C" int bcx_nuts_batch(void* stream, int32_t family, int32_t P, const bcx_nuts_problem* problems, void* table_dev, int32_t D,
                              int32_t chains, int32_t n_warmup, int32_t n_samples, int32_t max_depth, double eps0, const void* noise_dev,
                              int64_t noise_ld, int32_t ld, void* samples_dev, void* xi_dev, void* prop_dev, void* diag_dev, void* accept_dev,
                              void* eps_dev, void* status_dev, int32_t metric, void* frames_dev, void* metric_dev) {
  // what needs no device first: a caller without one reaches every one of these
  if (!hmc_common_ok(family, D, chains, n_warmup, n_samples, eps0, ld, noise_dev, samples_dev, diag_dev, accept_dev, eps_dev, status_dev) ||
      P < 1 || (int64_t)P * chains > INT32_MAX || !problems || !table_dev || max_depth < 1 || max_depth > NUTS_JMAX ||
      noise_ld < nuts_noise_row(D, max_depth) || (metric != 0 && metric != NUTS_METRIC_DIAG && metric != NUTS_METRIC_DENSE) ||
      (metric != 0) != (frames_dev != nullptr) || (metric != 0) != (metric_dev != nullptr))
    return bcx_fail(BCX_ERR_ARG, "bcx_nuts_batch", "bad arguments (those of bcx_nuts_coreset without fixed_eps; P >= 1 problems, P x chains "
                                                   "<= 2^31 - 1, problems and table_dev; metric 0 none / 1 diag / 2 dense, frames_dev and metric_dev iff a metric)");
  const int64_t row = D + (family == LAP_POISSON ? 1 : 0);
  for (int32_t p = 0; p < P; ++p) {
    const bcx_nuts_problem& q = problems[p];
    if (q.k < 0 || (q.W_dev && q.ldw < D) || (q.k > 0 && (!q.pts_dev || q.ldp < row)))
      return bcx_fail(BCX_ERR_ARG, "bcx_nuts_batch", "problem " + std::to_string(p) + ": bad arguments (k >= 0, ldw >= D with W_dev, pts_dev and "
                                                     "ldp >= the row with k > 0)");
  }
  // what asks the device: every problem within one workgroup's LDS, next to the static LDS of the kernel that runs
  int64_t lds = 0;
  for (int32_t p = 0; p < P; ++p) {
    const int32_t k = problems[p].k;
    const int64_t b = bcx_nuts_coreset_lds_bytes(k, D);
    if (!(metric ? bcx_nuts_adapt_ok(k, D) && nuts_batch_fits<true>(b) : bcx_nuts_coreset_ok(k, D) && nuts_batch_fits<false>(b)))
      return bcx_fail(BCX_ERR_ARG, "bcx_nuts_batch", "problem " + std::to_string(p) + ": " + std::to_string(k) + " points of " + std::to_string(D) +
                                                     " parameters are outside " + (metric ? "bcx_nuts_adapt_ok" : "bcx_nuts_coreset_ok"));
    if (b > lds) lds = b;
  }
  int win[2 * NUTS_ADAPT_WINDOWS] = {0};
  const int nwin = metric ? nuts_adapt_schedule(n_warmup, win, NUTS_ADAPT_WINDOWS) : 0;
  if (nwin > NUTS_ADAPT_WINDOWS) return bcx_fail(BCX_ERR_ARG, "bcx_nuts_batch", "more than 32 warm-up windows");
  // the dispatch order: k descending (the caller's order among equals), each record with its place in the caller's order
  std::vector<bcx_nuts_problem> table(problems, problems + P);
  for (int32_t p = 0; p < P; ++p) table[p].index = p;
  std::stable_sort(table.begin(), table.end(), [](const bcx_nuts_problem& x, const bcx_nuts_problem& y) { return x.k > y.k; });
  hipStream_t st = (hipStream_t)stream;
  // (the records are pageable host memory that ends with this call: the copy is waited for)
  BCX_TRY("bcx_nuts_batch", hipMemcpyAsync(table_dev, table.data(), (size_t)P * sizeof(bcx_nuts_problem), hipMemcpyHostToDevice, st));
  BCX_TRY("bcx_nuts_batch", hipStreamSynchronize(st));
  BCX_TRY("bcx_nuts_batch", hipMemset2DAsync(status_dev, 2 * sizeof(int), 0, sizeof(int), (size_t)P, st));      // status[2 p] of every problem
  NutsAdaptArgs g;
  NutsArgs& a = g.nuts;
  a.par = hmc_par(D, nullptr, nullptr, D, chains, n_warmup, n_samples, 0, eps0, 0.0, noise_dev, ld, samples_dev, xi_dev, prop_dev, diag_dev,
                  accept_dev, eps_dev, status_dev);
  a.w = nullptr; a.pts = nullptr; a.ldp = row; a.noise_ld = noise_ld; a.family = family; a.k = 0; a.J = max_depth;
  if (!metric) return nuts_batch_launch<false>(a, (const bcx_nuts_problem*)table_dev, P, chains, (size_t)lds, 16 * 1024, st);
  g.frames = (double*)frames_dev; g.metric_out = (double*)metric_dev; g.metric = metric; g.nwin = nwin;
  for (int i = 0; i < 2 * NUTS_ADAPT_WINDOWS; ++i) g.win[i] = win[i];
  return nuts_batch_launch<true>(g, (const bcx_nuts_problem*)table_dev, P, chains, (size_t)lds, 0, st);   // (its static LDS is past 48 KiB)
}
