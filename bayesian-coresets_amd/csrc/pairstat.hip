// pairstat.hip -- sums over all pairs of two sets of posterior draws, the two discrepancies the coreset papers report next to the
// moment errors (bayesiancoresets_amd/discrepancy.py): for rows a_i (i < nA) and b_j (j < nB) in D <= 32 coordinates
//     kind 0   sum_{i,j} |a_i - b_j|_2                                                     (the energy distance's three means)
//     kind 1   sum_{i,j} k_p(a_i, b_j), the Stein kernel of the IMQ base kernel (c^2 + |x - y|^2)^(-1/2) with scores g:
//              r = x - y, q = c^2 + |r|^2:   D q^(-3/2) - 3 |r|^2 q^(-5/2) - ((g_y - g_x) . r) q^(-3/2) + (g_x . g_y) q^(-1/2)
// Differences are formed coordinate by coordinate, r_k = x_k - y_k, and squared: never |x|^2 + |y|^2 - 2 x.y, whose cancellation
// turns the distance 0 of two equal draws (a rejected proposal repeats the state) into 1e-8 |x|.  So the work is on the fp64
// VALU -- the fp64 MFMA shares its datapath and rate (csrc/proj_math.h) and cannot form differences.
//
//   pair_tiles_kernel   a 256-thread workgroup owns 64 rows of A and walks one contiguous range of the 64-row tiles of B.  Both
//                       tiles (and their scores) lie in LDS k-major, s[k][row]; thread (ti, tj) = (t / 16, t % 16) owns the
//                       4 x 4 block of pairs rows 4 ti .. 4 ti + 3 of A against rows 4 tj .. 4 tj + 3 of B and reads, per k, four
//                       doubles of each operand once (16 lanes share an A address: a broadcast).  Per pair and k: kind 0 one
//                       subtract and one FMA; kind 1 two subtracts and three FMAs (|r|^2, g_x . g_y, (g_y - g_x) . r).  Then per
//                       pair one correctly rounded square root (kind 0) or one reciprocal square root and ten multiply-adds (kind
//                       1).  A thread adds its 16 values of a tile in block order, the tile's sum to its running sum, serially
//                       over the range; the workgroup adds its threads in a fixed tree (lanes by halving offsets, then the four
//                       waves in order) and writes ONE record (sum, sum of the terms i = j) per (A tile, range).
//   pair_total_kernel   one workgroup: thread t adds the records [n t / 256, n (t + 1) / 256) in index order, then the same tree.
//
// A against itself (B = NULL): only tiles j >= i are walked, a tile off the diagonal counts twice (an exact doubling), the
// diagonal tile is computed in full, and the terms i = j are summed besides (the U-statistic of discrepancy.py subtracts them).
// Rows past the end of a tile are staged as zeros and their pairs are SELECTED out (never multiplied by zero).  No floating-point
// atomics and every order fixed: two calls with the same arguments give the same bits.  Nothing is screened: a NaN anywhere is a
// NaN term and total; an infinite coordinate makes r infinite (kind 0: an infinite total; kind 1: 0 x inf = NaN) or, against
// itself or an equal infinity, inf - inf = NaN.
//
// Bound: the fp64 VALU.  Per pair 2 D (kind 0) or 5 D (kind 1) lane-operations in the loop and about 20 behind it, against
// 256 CUs x 4 SIMDs x 16 fp64 lanes per clock.  LDS: eight (kind 0: four) 16-byte reads per thread and k feed
// 80 (32) VALU instructions.  Measured on an MI355X (tools/discrepancy_bench.py): 0.55 - 0.65 of that ceiling from
// 32 768 draws a side on; the staging of a tile is not overlapped with the arithmetic.
#include <math.h>
#include <string>
#include "bcx_internal.h"
#include "launch_host.h"

#define PS_DMAX 32
#define PS_TILE 64                 // rows of a tile, both sides
#define PS_BLK 4                   // a thread's block of pairs is PS_BLK x PS_BLK
#define PS_MAX_SPLITS 1024
#define PS_MAX_ROWS ((int64_t)1 << 20)

typedef double ps4d __attribute__((ext_vector_type(4)));

struct PairArgs {
  const double* A;      // nA x lda
  const double* GA;     // nA x ldga (kind 1)
  const double* B;      // nB x ldb  (A itself when sym)
  const double* GB;     // nB x ldgb (kind 1)
  double* rec;          // tiles of A x ranges x 2
  int64_t nA, lda, ldga, nB, ldb, ldgb;
  double c2, Dd;        // c^2 and D as a double
  int D, ranges, sym;
};

// 64 rows of P from row0 on into s[k][row]; rows from n on are zeros (their address is row 0's: n >= 1).  Four lanes share a row.
static __device__ __forceinline__ void ps_stage(double* s, const double* P, int64_t ld, int64_t row0, int64_t n, int D) {
  const int row = threadIdx.x >> 2, kq = threadIdx.x & 3;
  const bool ok = row0 + row < n;
  const double* p = P + (ok ? row0 + row : 0) * ld;
  for (int k = kq; k < D; k += 4) {
    const double v = p[k];
    s[k * PS_TILE + row] = ok ? v : 0.0;
  }
}

// the workgroup's (x, y) in thread 0: lanes by halving offsets, the four waves in order.  `s` is LDS nobody reads any more.
static __device__ __forceinline__ void ps_reduce(double& x, double& y, double* s) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    x += __shfl_down(x, off);
    y += __shfl_down(y, off);
  }
  __syncthreads();
  if ((threadIdx.x & 63) == 0) { s[2 * (threadIdx.x >> 6)] = x; s[2 * (threadIdx.x >> 6) + 1] = y; }
  __syncthreads();
  if (threadIdx.x == 0) {
    x = s[0]; y = s[1];
    for (int w = 1; w < 4; ++w) { x += s[2 * w]; y += s[2 * w + 1]; }
  }
}

template <int KIND>
__global__ __launch_bounds__(256) void pair_tiles_kernel(PairArgs a) {
  __shared__ __attribute__((aligned(32))) double smem[(KIND == 1 ? 4 : 2) * PS_DMAX * PS_TILE];
  double* const sA = smem;
  double* const sB = smem + PS_DMAX * PS_TILE;
  double* const sGA = smem + 2 * PS_DMAX * PS_TILE;       // (kind 1 only)
  double* const sGB = smem + 3 * PS_DMAX * PS_TILE;
  const int ti = threadIdx.x >> 4, tj = threadIdx.x & 15;
  const int D = a.D;
  const int64_t ta = blockIdx.x;
  const int64_t tiles_b = (a.nB + PS_TILE - 1) / PS_TILE;
  const int64_t first = a.sym ? ta : 0, span = tiles_b - first;
  const int64_t t_begin = first + span * (int64_t)blockIdx.y / a.ranges, t_end = first + span * ((int64_t)blockIdx.y + 1) / a.ranges;

  ps_stage(sA, a.A, a.lda, ta * PS_TILE, a.nA, D);
  if (KIND == 1) ps_stage(sGA, a.GA, a.ldga, ta * PS_TILE, a.nA, D);
  bool oka[PS_BLK];
#pragma unroll
  for (int i = 0; i < PS_BLK; ++i) oka[i] = ta * PS_TILE + PS_BLK * ti + i < a.nA;

  double acc = 0.0, dacc = 0.0;
  for (int64_t tb = t_begin; tb < t_end; ++tb) {
    __syncthreads();                                      // (the readers of the previous tile)
    ps_stage(sB, a.B, a.ldb, tb * PS_TILE, a.nB, D);
    if (KIND == 1) ps_stage(sGB, a.GB, a.ldgb, tb * PS_TILE, a.nB, D);
    __syncthreads();
    double d2[PS_BLK][PS_BLK], gg[PS_BLK][PS_BLK], gr[PS_BLK][PS_BLK];
#pragma unroll
    for (int i = 0; i < PS_BLK; ++i)
#pragma unroll
      for (int j = 0; j < PS_BLK; ++j) d2[i][j] = gg[i][j] = gr[i][j] = 0.0;
    for (int k = 0; k < D; ++k) {
      const ps4d xa = *(const ps4d*)(sA + k * PS_TILE + PS_BLK * ti);
      const ps4d xb = *(const ps4d*)(sB + k * PS_TILE + PS_BLK * tj);
      if (KIND == 1) {
        const ps4d ga = *(const ps4d*)(sGA + k * PS_TILE + PS_BLK * ti);
        const ps4d gb = *(const ps4d*)(sGB + k * PS_TILE + PS_BLK * tj);
#pragma unroll
        for (int i = 0; i < PS_BLK; ++i)
#pragma unroll
          for (int j = 0; j < PS_BLK; ++j) {
            const double r = xa[i] - xb[j], dg = gb[j] - ga[i];
            d2[i][j] = fma(r, r, d2[i][j]);
            gg[i][j] = fma(ga[i], gb[j], gg[i][j]);
            gr[i][j] = fma(dg, r, gr[i][j]);
          }
      } else {
#pragma unroll
        for (int i = 0; i < PS_BLK; ++i)
#pragma unroll
          for (int j = 0; j < PS_BLK; ++j) {
            const double r = xa[i] - xb[j];
            d2[i][j] = fma(r, r, d2[i][j]);
          }
      }
    }
    const bool on_diag = a.sym && tb == ta;
    double ts = 0.0;
#pragma unroll
    for (int i = 0; i < PS_BLK; ++i)
#pragma unroll
      for (int j = 0; j < PS_BLK; ++j) {
        double term;
        if (KIND == 1) {
          const double q = a.c2 + d2[i][j];
          const double rs = rsqrt(q);
          const double rs2 = rs * rs, rs3 = rs2 * rs;
          const double u = (a.Dd - gr[i][j]) * rs3;
          const double v = (3.0 * d2[i][j]) * (rs3 * rs2);
          term = fma(gg[i][j], rs, u) - v;
        } else {
          term = sqrt(d2[i][j]);
        }
        const bool ok = oka[i] && tb * PS_TILE + PS_BLK * tj + j < a.nB;
        term = ok ? term : 0.0;
        ts += term;
        if (KIND == 1 && i == j) dacc += (on_diag && ti == tj) ? term : 0.0;
      }
    acc += (a.sym && tb != ta) ? 2.0 * ts : ts;
  }
  ps_reduce(acc, dacc, smem);
  if (threadIdx.x == 0) {
    double* o = a.rec + ((size_t)ta * (size_t)a.ranges + blockIdx.y) * 2;
    o[0] = acc; o[1] = dacc;
  }
}

__global__ __launch_bounds__(256) void pair_total_kernel(const double* __restrict__ rec, int64_t n, double* __restrict__ out) {
  __shared__ double s[8];
  const int64_t b = n * (int64_t)threadIdx.x / 256, e = n * ((int64_t)threadIdx.x + 1) / 256;
  double x = 0.0, y = 0.0;
  for (int64_t i = b; i < e; ++i) { x += rec[2 * i]; y += rec[2 * i + 1]; }
  ps_reduce(x, y, s);
  if (threadIdx.x == 0) { out[0] = x; out[1] = y; }
}

// ranges of B's tiles per tile of A: the caller's count, or enough workgroups to fill the device a few times over
static int ps_ranges(int64_t tiles_a, int64_t tiles_b, int splits) {
  if (splits > 0) return splits;
  const int cus = cu_count();
  int64_t want = ((int64_t)8 * cus + tiles_a - 1) / tiles_a;
  if (want > tiles_b) want = tiles_b;
  if (want > PS_MAX_SPLITS) want = PS_MAX_SPLITS;
  return want < 1 ? 1 : (int)want;
}
static bool ps_shape_ok(int64_t nA, int64_t nB, int32_t D, int32_t splits) {
  return nA >= 1 && nA <= PS_MAX_ROWS && nB >= 0 && nB <= PS_MAX_ROWS && D >= 1 && D <= PS_DMAX && splits >= 0 && splits <= PS_MAX_SPLITS;
}

extern "C" int64_t bcx_pair_stat_scratch_bytes(int64_t nA, int64_t nB, int32_t D, int32_t splits) {
  if (!ps_shape_ok(nA, nB, D, splits)) return -1;
  const int64_t tiles_a = (nA + PS_TILE - 1) / PS_TILE, tiles_b = ((nB ? nB : nA) + PS_TILE - 1) / PS_TILE;
  return tiles_a * ps_ranges(tiles_a, tiles_b, splits) * 2 * (int64_t)sizeof(double);
}
extern "C" int bcx_pair_stat(void* stream, int32_t kind, const void* A_dev, int64_t nA, int64_t lda, const void* GA_dev, int64_t ldga,
                             const void* B_dev, int64_t nB, int64_t ldb, const void* GB_dev, int64_t ldgb, int32_t D, double c,
                             int32_t splits, void* out_dev, void* work_dev, int64_t work_bytes) {
  const bool sym = B_dev == nullptr;
  if (sym) { nB = 0; ldb = lda; ldgb = ldga; }
  if ((kind != 0 && kind != 1) || !ps_shape_ok(nA, nB, D, splits) || !A_dev || lda < D || (!sym && (nB < 1 || ldb < D)) ||
      (kind == 1 && (!GA_dev || ldga < D || !(c > 0.0) || !(c < INFINITY) || (!sym && (!GB_dev || ldgb < D)))) || !out_dev || !work_dev ||
      work_bytes < bcx_pair_stat_scratch_bytes(nA, nB, D, splits))
    return bcx_fail(BCX_ERR_ARG, "bcx_pair_stat", "bad arguments (kind 0 distances / 1 Stein terms, 1 <= rows <= 2^20 a side, 1 <= D <= 32, row "
                                                  "strides >= D, scores and a finite c > 0 for kind 1, 0 <= splits <= 1024, work_dev of "
                                                  "bcx_pair_stat_scratch_bytes)");
  hipStream_t st = (hipStream_t)stream;
  PairArgs a;
  a.A = (const double*)A_dev; a.GA = (const double*)GA_dev; a.nA = nA; a.lda = lda; a.ldga = ldga;
  a.B = sym ? a.A : (const double*)B_dev; a.GB = sym ? a.GA : (const double*)GB_dev; a.nB = sym ? nA : nB; a.ldb = ldb; a.ldgb = ldgb;
  a.rec = (double*)work_dev; a.c2 = c * c; a.Dd = (double)D; a.D = D; a.sym = sym ? 1 : 0;
  const int64_t tiles_a = (nA + PS_TILE - 1) / PS_TILE, tiles_b = (a.nB + PS_TILE - 1) / PS_TILE;
  a.ranges = ps_ranges(tiles_a, tiles_b, splits);
  const dim3 grid((unsigned)tiles_a, (unsigned)a.ranges);
  if (kind == 1) hipLaunchKernelGGL(pair_tiles_kernel<1>, grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL(pair_tiles_kernel<0>, grid, dim3(256), 0, st, a);
  hipLaunchKernelGGL(pair_total_kernel, dim3(1), dim3(256), 0, st, (const double*)work_dev, tiles_a * (int64_t)a.ranges, (double*)out_dev);
  BCX_TRY("bcx_pair_stat", hipGetLastError());
  return BCX_OK;
}
