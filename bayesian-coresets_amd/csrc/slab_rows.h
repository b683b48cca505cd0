// slab_rows.h -- the two pieces that the slabbed matrix-vector pairs over the k x S projected coreset points share
// (csrc/svi.hip svi_adam_a / b_kernel: resid and gradient of SparseVI's ADAM step; csrc/qn.hip qn_center / qn_rhs_kernel: resid
// and right-hand side of the quasi-Newton step).  One workgroup of 256 threads per slab of ROWS points; every loop keeps its
// loads independent and in flight together, every sum has one fixed order.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// t[u] = this lane's share of the sum of row j0 + wave + 4 u over the S draws (zero for rows the slab does not have, or when
// the rows arrive centred): the rows of a wave are requested together.  The caller adds the lanes (wave_allsum) and divides.
template <int ROWS>
static __device__ __forceinline__ void slab_row_sums(const double* __restrict__ core, int64_t ldc, int j0, int nj, int S, bool raw,
                                                     double (&t)[ROWS / 4]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int u = 0; u < ROWS / 4; ++u) {
    const int q = wave + 4 * u;
    t[u] = 0.0;
    if (raw && q < nj) {
      const double* row = core + (size_t)(j0 + q) * ldc;
      for (int s = lane; s < S; s += 64) t[u] += row[s];
    }
  }
}

// Column s of the slabs' shares (part: nslab x S), added in slab order: thirty-two shares in flight (300 weights: ONE round
// trip), then eight, then one.
static __device__ __forceinline__ double slab_share_sum(const double* __restrict__ part, int nslab, int S, int s) {
  double t = 0.0;
  int b = 0;
  for (; b + 32 <= nslab; b += 32) {
    double v[32];
#pragma unroll
    for (int q = 0; q < 32; ++q) v[q] = part[(size_t)(b + q) * S + s];
#pragma unroll
    for (int q = 0; q < 32; ++q) t += v[q];
  }
  for (; b + 8 <= nslab; b += 8) {
    double v[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) v[q] = part[(size_t)(b + q) * S + s];
#pragma unroll
    for (int q = 0; q < 8; ++q) t += v[q];
  }
  for (; b < nslab; ++b) t += part[(size_t)b * S + s];
  return t;
}
