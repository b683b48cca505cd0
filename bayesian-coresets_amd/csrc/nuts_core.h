// nuts_core.h -- what the two NUTS kernels share (csrc/nuts.hip: the points in one workgroup's LDS; csrc/nuts_stream.hip: the
// rows streamed by a persistent grid): the limits, the tree's storage and the two scalar functions of the transition.
#pragma once
#include "hmc_core.h"

#define NUTS_JMAX 10
#define NUTS_DIAG 8
#define NUTS_DIVERGENT -1000.0

struct NutsTree {
  double xl[32], pl[32], gl[32], xr[32], pr[32], gr[32];     // the tree's endpoints: xi, momentum, xi-gradient
  double gm[32];                                             // the xi-gradient at the moving end (its xi and momentum: S.s.xp, S.s.p)
  double xs[32], gs[32], ths[32];                            // the doubling's proposal: xi, xi-gradient, theta
  double ckx[NUTS_JMAX][32], ckp[NUTS_JMAX][32];             // checkpoints: xi and momentum of even leaves, slot popcount(leaf)
};

static __device__ __forceinline__ double nuts_logaddexp(double a, double b) { return fmax(a, b) + log1p(exp(-fabs(a - b))); }
static __device__ __forceinline__ double nuts_threshold(const double* z) { return 0.5 * (z[0] * z[0] + z[1] * z[1]); }

// standard normals one NUTS transition reads with J = max_depth (1 .. NUTS_JMAX): D momenta, three per doubling, two per leaf slot
static inline int64_t nuts_noise_row(int32_t D, int32_t J) { return (int64_t)D + 3 * (int64_t)J + 2 * (((int64_t)1 << J) - 1); }
