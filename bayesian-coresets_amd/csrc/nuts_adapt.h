// nuts_adapt.h -- the windowed metric adaptation of the LDS-resident NUTS kernel (csrc/nuts.hip): the schedule of
// the warm-up windows (host), the running mean and sum of outer products of a window's draws, and what the end of a window does.
//
// A metric M^-1 = L L^T in xi0 coordinates (theta = mu + W0^T xi0, W0 the frame the caller passed) is a unit metric in eta,
// xi0 = L eta, theta = mu + (L^T W0)^T eta: the transition of csrc/nuts.hip runs unchanged in eta with the frame S.W = L^T W0.
// Only S.W, the chain's coordinate and its carried gradient change, per chain, at the end of a window.
#pragma once
#include "hmc_core.h"
#include "chol32.h"

#define NUTS_ADAPT_WINDOWS 32
enum { NUTS_METRIC_DIAG = 1, NUTS_METRIC_DENSE = 2 };

struct NutsAdaptLds {
  double W0[32 * HMC_LDW];   // the frame the caller passed
  double L[32 * HMC_LDW];    // lower triangular, identity at the start and beyond D
  double M2[32 * HMC_LDW];   // lower triangle: sum of outer products about the running mean; at a window's end X = L^-T
  double mean[32], x0[32];   // the running mean; xi0 = L eta of the newest draw
  int ok;
};

// The slow windows [start, end) of a warm-up of n_warmup transitions (Stan's three phases: 75 fast, windows doubling from 25, 50
// fast; 15 % / 75 % / 10 % when that does not fit; none below 20): writes up to `cap` pairs, returns the number of windows.
static inline int nuts_adapt_schedule(int32_t n_warmup, int32_t* bounds, int32_t cap) {
  if (n_warmup < 20) return 0;
  int64_t init = 75, term = 50, base = 25;
  if (init + term + base > n_warmup) {
    init = (int64_t)n_warmup * 15 / 100;
    term = (int64_t)n_warmup / 10;
    base = n_warmup - init - term;
  }
  const int64_t stop = n_warmup - term;
  int n = 0;
  for (int64_t s = init, w = base; s < stop; w *= 2) {
    int64_t e = s + w;
    if (e + 2 * w > stop) e = stop;
    if (n < cap && bounds) { bounds[2 * n] = (int32_t)s; bounds[2 * n + 1] = (int32_t)e; }
    ++n;
    s = e;
  }
  return n;
}

static __device__ __forceinline__ void nuts_adapt_init(NutsAdaptLds& A, const HmcLds& S) {
  for (int e = threadIdx.x; e < 32 * HMC_LDW; e += blockDim.x) {
    const int i = e / HMC_LDW, c = e - i * HMC_LDW;
    A.W0[e] = S.W[e];
    A.L[e] = i == c ? 1.0 : 0.0;
    A.M2[e] = 0.0;
  }
  if (threadIdx.x < 32) { A.mean[threadIdx.x] = 0.0; A.x0[threadIdx.x] = 0.0; }
  if (threadIdx.x == 0) A.ok = 1;
}

// The state S.s.xi joins the window as its n-th draw (n = 1, 2, ..): x = L eta, then Welford's update with one thread per entry,
//   d = x - mean;  mean' = mean + d / n;  M2 += d (x - mean')^T.   Leaves x in A.x0 and the block synchronised.
static __device__ __forceinline__ void nuts_adapt_accumulate(NutsAdaptLds& A, const HmcLds& S, int D, int n) {
  const int tid = threadIdx.x;
  if (tid < 32) {
    double v = 0.0;
    if (tid < D) for (int j = 0; j <= tid; ++j) v = fma(A.L[tid * HMC_LDW + j], S.s.xi[j], v);
    A.x0[tid] = v;
  }
  __syncthreads();
  const double dn = (double)n;
  for (int e = tid; e < 32 * 32; e += HMC_THREADS) {
    const int i = e >> 5, j = e & 31;
    if (i < D && j <= i) {
      const double di = A.x0[i] - A.mean[i], dj = A.x0[j] - A.mean[j];
      const double mj = A.mean[j] + dj / dn;
      A.M2[i * HMC_LDW + j] += di * (A.x0[j] - mj);
    }
  }
  __syncthreads();
  if (tid < D) A.mean[tid] += (A.x0[tid] - A.mean[tid]) / dn;
  __syncthreads();
}

// The end of a window of n draws, the newest still in A.x0.  Sigma = n / (n + 5) S + 1e-3 * 5 / (n + 5) I with S the sample
// covariance (ddof 1; its diagonal alone in diag mode), L = chol(Sigma) by one wave, then eta = L^-1 x0 into S.s.xi and
// S.W = L^T W0.  A pivot that is not positive and finite keeps L, S.W and S.s.xi as they are.  The accumulators are cleared
// either way.  Returns whether the frame changed; leaves the block synchronised.  The caller evaluates the target at the state.
static __device__ __forceinline__ bool nuts_adapt_window_end(NutsAdaptLds& A, HmcLds& S, int D, int n, int metric) {
  const int tid = threadIdx.x;
  const double dn = (double)n;
  const double c1 = dn / (dn + 5.0), c2 = 1e-3 * (5.0 / (dn + 5.0));
  if (tid < 64) {
    const int row = tid & 31;
    const bool top = tid < 32;
    if (metric == NUTS_METRIC_DENSE) {
      double r[32];
#pragma unroll
      for (int c = 0; c < 32; ++c) {
        const double sig = c1 * (A.M2[row * HMC_LDW + c] / (dn - 1.0)) + (c == row ? c2 : 0.0);
        r[c] = (top && row < D) ? (c <= row ? sig : 0.0) : (c == row ? 1.0 : 0.0);
      }
      double dmin;
      chol32_factor(r, dmin);
      const bool ok = dmin > 0.0 && dmin < INFINITY;
      if (ok) {
        // lanes 0 .. 31: rows of L (what the column operations left right of the diagonal is not part of it);
        // lanes 32 .. 63: rows of X = L^-T, upper triangular, into the accumulator's place (every lane has read its row)
        double* dst = top ? A.L : A.M2;
#pragma unroll
        for (int c = 0; c < 32; ++c) dst[row * HMC_LDW + c] = (top ? c <= row : c >= row) ? r[c] : 0.0;
      }
      if (tid == 0) A.ok = ok ? 1 : 0;
    } else {
      const double sig = (top && row < D) ? c1 * (A.M2[row * HMC_LDW + row] / (dn - 1.0)) + c2 : 1.0;
      const bool ok = !__any(!(sig > 0.0 && sig < INFINITY));
      if (ok && top) A.L[row * HMC_LDW + row] = sqrt(sig);
      if (tid == 0) A.ok = ok ? 1 : 0;
    }
  }
  __syncthreads();
  const bool ok = A.ok != 0;
  if (ok) {
    if (tid < D) {
      double v;
      if (metric == NUTS_METRIC_DENSE) {
        v = 0.0;
        for (int j = 0; j <= tid; ++j) v = fma(A.M2[j * HMC_LDW + tid], A.x0[j], v);      // L^-1[i][j] = X[j][i]
      } else {
        v = A.x0[tid] / A.L[tid * HMC_LDW + tid];
      }
      S.s.xi[tid] = v;
    }
    for (int e = tid; e < 32 * 32; e += HMC_THREADS) {
      const int i = e >> 5, c = e & 31;
      if (i < D && c < D) {
        double v = 0.0;
        for (int j = i; j < D; ++j) v = fma(A.L[j * HMC_LDW + i], A.W0[j * HMC_LDW + c], v);
        S.W[i * HMC_LDW + c] = v;
      }
    }
  }
  __syncthreads();
  for (int e = tid; e < 32 * HMC_LDW; e += HMC_THREADS) A.M2[e] = 0.0;
  if (tid < 32) A.mean[tid] = 0.0;
  __syncthreads();
  return ok;
}
