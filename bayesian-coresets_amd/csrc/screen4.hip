// screen4.hip -- a 4-bit front pass in front of the 8-bit screening tier (single-query algorithms: FW, OMP; one shard).
//
// The 8-bit tier (screen8.hip) streams one byte per element every greedy iteration and runs at the HBM rate: the step is the
// bytes of its shadow.  This file keeps a second, coarser shadow of half a byte per element and streams THAT; the 8-bit
// shadow is then read only for the rows the coarse pass cannot exclude.  What makes four bits enough is that the cut-off is
// known BEFORE the pass: the lower bound of any row is a lower bound of the maximum, so a handful of rows that led the
// previous iteration ("sentinels"), scored in 8 bits against the new query, give a threshold Lg, and a row whose 4-bit UPPER
// bound is below Lg is out -- only the one-sided 4-bit error enters.  A poor threshold lists more rows; it never changes
// the result.  One 4-bit iteration is three launches (front pass, refine, tail):
//
//   (refine_kernel of the PREVIOUS iteration, screen8.hip): it holds the tier's partials, which name two rows per wave with
//                    their 8-bit upper bounds; each of its 16 waves takes the 4 largest among the candidates it holds (64
//                    "sentinel" rows; among them the 4 largest overall) and leaves their indices in a 64-word buffer.
//   front4_kernel  : every workgroup first computes the head of the pass for itself (front4_head) while the loads of its
//                    first trip are in flight: no launch of its own, and no workgroup waits for another.
//                    (a) The fp32 query q~ becomes integers x_j = rint(q~_j / qstep) in [-1911, 1911],
//                    qstep = max|q~| / 1911, written as three planes of signed nibbles x = 256 h2 + 16 h1 + l, each digit
//                    in [-8, 7], eight elements per dword -- the operand format of v_dot8_i32_i4 -- to LDS, from where
//                    every lane takes the dwords of its own pieces.  qerr is an fp32 round-up of || q~ - x qstep ||_2
//                    summed in fp64.  (b) Each sentinel is scored from the 8-bit shadow against the new query (products
//                    exact, sum in fp64; 16 rows per wave, 33 KB at d = 512 that all but the first reader find in L2)
//                    and gets screen_interval's lower bound, the one screen_kernel would give it; Lg is their maximum.
//                    All workgroups compute bit-identical Lg, qstep and coefficients of e4: there is one Lg.
//                    Then screen_kernel's streaming structure (16-byte non-temporal loads, G lanes per row, <= 512 workgroups)
//                    over the 4-bit codes, without tracks.  A dword holds eight codes c + 8, element 8 w + k in bits 4k..4k+3;
//                    xor 0x88888888 turns them into two's-complement nibbles, three v_dot8_i32_i4 against the query planes
//                    give exact integer sums (|sum| <= 4096 * 7 * 1911 < 2^26), 4 instructions per 8 elements.
//                      score4 = scale4 * qstep * sum_j c_j x_j ,   U4 = score4 + e4
//                    A row with not (U4 < Lg) is appended to the wave's own segment of the list buffer (BCX_S4_SEG_CAP
//                    entries; ballot + prefix count, the fill count stays in a register, no atomics).  A wave that wanted
//                    to list more says so by its count.
//                    Second stage, same launch (settle8): a wave that has finished its stream reads its own segment (from
//                    a copy in LDS: 4 x 4 KB) and gives the listed rows screen_kernel's 8-bit score and interval (the
//                    device functions of screen_core.h, same lane layout, so kacc holds as derived there), tracks top-2 /
//                    U3 / L and writes partial w of scr_partials in screen_kernel's format; its gathers run beside the
//                    streams of the waves that are still at it.  A wave whose segment overflowed writes the partial that
//                    makes refine_kernel report an overflow.
//   refine_kernel  : as after the 8-bit pass; resolve_core, the fp64 re-score and the tail follow unchanged.  It also books
//                    this tier's counters from the list counts and picks the next iteration's sentinels from the partials.
//
// The enclosure of the front pass.  a*: exact normalised row, a~: stored row, deq4_j = c_j scale4, q*: exact query, q~: the
// fp32 query, qu_j = x_j qstep, qs = |q~| (DevState::qscale), s* = a* . q*:
//   |score4 - s*| <= |score4 - deq4.qu| + |deq4.(qu - q~)| + |(deq4 - a~).q~| + |a~.q~ - s*|
//   (4) storage rounding of row and query:                <= err_coef * qs          (bcx_scan_plan's term, as in screen8.hip)
//   (3) Cauchy-Schwarz, bound4 >= ||a~ - deq4||_2 from the quantiser (clipping included: it is summed from the stored row)
//                                                          <= bound4 * qs
//   (2) ||deq4|| <= ||a~|| + bound4 <= 1.001 + bound4:     <= (1.001 + bound4) * qerr
//   (1) the integer sum is exact; int -> fp32 and two multiplies round by 3 u |score4| in all, u = 2^-24
//   e4 = bound4 * eA + eB + 5e-7 |score4|,   eA = (qs (1 + 2e-6) + qerr)(1 + 4e-6),
//                                            eB = (err_coef qs + 1.001 qerr)(1 + 4e-6) + 1e-37   (both rounded up to fp32;
//   the factors cover the fp32 rounding of qs, of e4's own fused multiply-add and of the final sum U4 = score4 + e4).
// With 12 query bits qerr is about 3e-4 qs for a random query, next to bound4 ~ 0.11: the query costs nothing.
// tests/test_screen4_bound.py restates quantiser and e4 in NumPy; tools/screen4_model.py gives the listed fractions, the
// fullest segment and the redos from which c = BCX_S4_CLIP and BCX_S4_SEG_CAP were chosen.
#include <float.h>
#include "screen_core.h"

#define BCX_S4_CLIP 0.8          // scale4 = BCX_S4_CLIP * max|a| / 7, codes clipped to [-7, 7]
#define BCX_S4_QMAX 1911.0       // 7 * (256 + 16 + 1): the largest integer three digits in [-8, 7] reach on both sides
#define BCX_S4_MAX_NW4 512       // dwords of a 4-bit row at d = 4096, the longest row the tier takes

struct Front4Head { float Lg, qstep, eA, eB; };   // (registers of every thread of the front pass; never in memory)

// ---- cross-lane integer sum over groups of G lanes (the DPP / permlane-swap steps of scan_core.h on integers) -------------
template <int CTRL> __device__ __forceinline__ int dpp_mov_i(int v) { return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xf, 0xf, false); }
template <int G> __device__ __forceinline__ int group_allsum_i32(int v) {
  if (G >= 2) v += dpp_mov_i<0xB1>(v);
  if (G >= 4) v += dpp_mov_i<0x4E>(v);
  if (G >= 8) v += dpp_mov_i<0x141>(v);
  if (G >= 16) v += dpp_mov_i<0x140>(v);
  if (G >= 32) { const v2u r = __builtin_amdgcn_permlane16_swap((unsigned)v, (unsigned)v, false, false); const unsigned x = r.x, y = r.y; v = (int)(x + y); }
  if (G >= 64) { const v2u r = __builtin_amdgcn_permlane32_swap((unsigned)v, (unsigned)v, false, false); const unsigned x = r.x, y = r.y; v = (int)(x + y); }
  return v;
}

static __device__ __forceinline__ float round_up_f32(double v) {
  float f = (float)v;
  if ((double)f < v) f = nextafterf(f, INFINITY);
  return f;
}

// ---- front pass -------------------------------------------------------------------------------------------------------------
struct Front4Args {
  const uint4* A4;      // n x ldv pieces of 32 codes
  const float2* sb;     // per row: (scale4, bound4)
  const float* q;       // the fp32 query
  const int* sent;      // BCX_S4_SENTINELS row indices the previous iteration's refine_kernel left, -1: none
  const unsigned char* Aq;   // 8-bit shadow and its (scale, bound): the sentinels are scored from it
  const float2* sb8;
  const DevState* st;
  int* list;            // one segment of BCX_S4_SEG_CAP entries per wave, of which seg_cap are in use
  int* counts;          // rows the wave wanted to list
  int64_t n;
  int ldv, nw4, seg_cap;
  int ld8, d;
  float kacc, err_coef; // of the 8-bit tier (screen_interval)
  PartialView out;      // one partial per wave, screen_kernel's format: the listed rows settled in 8 bits
  int ldv8;             // 16-byte pieces of an 8-bit row
};

#define BCX_S4_SPW (BCX_S4_SENTINELS / BCX_SCREEN_WAVES)   // sentinel rows a wave of the front pass scores

// The head of one front pass: threshold, query step and the two coefficients of e4.  Called by all BCX_SCAN_THREADS threads of a
// workgroup; lane l of a wave brings sentinel row l mod 16 of the wave's 16 (-1: none) and that row's (scale, bound).  It also
// leaves the query's three nibble planes (nw4 dwords each) in `planes`, published by its barrier.
// Every workgroup runs this text on the same inputs with the same reduction order (lane-strided sums, the butterfly inside a
// wave, waves 0..3 in turn), so all of them hold bit-identical Lg / qstep / eA / eB and planes: there is one Lg, and the list
// is what one threshold kernel in front of the pass would have given.
// Its time is latency, so the loads are vector loads that are in flight together (the rows' codes two strides of the lanes per
// trip), and the scores come before the first barrier.
static __device__ __forceinline__ Front4Head front4_head(const Front4Args& a, int myrow, float2 mysb, float qscale,
                                                         unsigned* planes, double* scratch) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  constexpr int NW = BCX_SCREEN_WAVES;
  constexpr int SPW = BCX_S4_SPW;
  int rows[SPW];        // (wave-uniform)
#pragma unroll
  for (int r = 0; r < SPW; ++r) rows[r] = __builtin_amdgcn_readlane(myrow, r);
  // (b) this wave's sentinels' 8-bit scores against the new query (products exact, sum in fp64, a lane's words in ascending
  // order; a word beyond the row meets a zero query)
  // (a) on the way, the query's largest magnitude: a wave's lanes read all of the query here, so every wave has it whole
  double acc[SPW];
#pragma unroll
  for (int r = 0; r < SPW; ++r) acc[r] = 0.0;
  double m = 0.0;
  const int nw8 = a.ld8 / 4;
  const unsigned* A8 = (const unsigned*)a.Aq;
  for (int w0 = lane; w0 < nw8; w0 += 128) {
    unsigned cw[2][SPW];
    float qf[2][4];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int w = w0 + 64 * h;
      const int wc = w < nw8 ? w : 0;
#pragma unroll
      for (int k = 0; k < 4; ++k) { const int j = 4 * w + k; qf[h][k] = a.q[(w < nw8 && j < a.d) ? j : 0]; }
#pragma unroll
      for (int r = 0; r < SPW; ++r) cw[h][r] = A8[(int64_t)(rows[r] < 0 ? 0 : rows[r]) * nw8 + wc];
    }
    __builtin_amdgcn_sched_barrier(0);   // all of the trip's loads in flight before the first use
    double qv[2][4];
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int w = w0 + 64 * h, j = 4 * w + k;
        qv[h][k] = (w < nw8 && j < a.d) ? (double)qf[h][k] : 0.0;
        const double v = fabs(qv[h][k]);
        m = fmax(m, v == v ? v : INFINITY);
      }
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int r = 0; r < SPW; ++r)
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[r] = fma((double)((int)((cw[h][r] >> (8 * k)) & 0xffu) - 128), qv[h][k], acc[r]);
  }
  double tot = 0.0;     // of this lane's own row
#pragma unroll
  for (int r = 0; r < SPW; ++r) { const double t = wave_allsum(acc[r]); tot = (lane & (SPW - 1)) == r ? t : tot; }
  float lmax = -INFINITY;
  {
    const float s0 = (float)((double)mysb.x * tot);    // one rounding, inside the 2e-7 |s| of screen_interval
    float U, L;
    screen_interval(s0, mysb.x, mysb.y, a.kacc, a.err_coef, qscale, U, L);
    if (myrow >= 0) lmax = fmaxf(lmax, L);             // (a NaN bound is no bound: fmaxf drops it)
  }
  lmax = (float)wave_allmax((double)lmax);
  m = wave_allmax(m);   // -> the query's step
  float step = (float)(m / BCX_S4_QMAX);
  const bool qok = m < INFINITY && step >= FLT_MIN;   // else: nothing is excluded this iteration (Lg = -inf)
  if (!qok) step = 0.0f;
  // (c) the query in three nibble planes, and its squared rounding error
  double err2 = 0.0;
  for (int w = tid; w < a.nw4; w += BCX_SCAN_THREADS) {
    unsigned p0 = 0, p1 = 0, p2 = 0;
    float q8[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) { const int j = 8 * w + k; q8[k] = a.q[j < a.d ? j : 0]; }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int j = 8 * w + k;
      int x = 0;
      if (j < a.d && qok) {
        const double v = (double)q8[k];
        double c = rint(v / (double)step);
        c = c > BCX_S4_QMAX ? BCX_S4_QMAX : (c < -BCX_S4_QMAX ? -BCX_S4_QMAX : c);
        x = (int)c;
        const double r = v - c * (double)step;
        err2 = fma(r, r, err2);
      }
      const int l = ((x + 8) & 15) - 8;
      const int x1 = (x - l) >> 4;
      const int h1 = ((x1 + 8) & 15) - 8;
      const int h2 = (x1 - h1) >> 4;
      p0 |= (unsigned)(l & 15) << (4 * k); p1 |= (unsigned)(h1 & 15) << (4 * k); p2 |= (unsigned)(h2 & 15) << (4 * k);
    }
    planes[w] = p0; planes[a.nw4 + w] = p1; planes[2 * a.nw4 + w] = p2;
  }
  err2 = wave_allsum(err2);
  if (lane == 0) { scratch[wave] = err2; scratch[NW + wave] = (double)lmax; }
  __syncthreads();                                    // (also publishes the planes)
  err2 = scratch[0];
  double lg = scratch[NW];
#pragma unroll
  for (int w = 1; w < NW; ++w) { err2 += scratch[w]; lg = fmax(lg, scratch[NW + w]); }
  const double qerr = sqrt(err2) * (1.0 + 9.5367431640625e-07);
  const double qs = (double)qscale;
  Front4Head h;
  h.Lg = qok ? (float)lg : -INFINITY;
  h.qstep = step;
  h.eA = round_up_f32((qs * 1.000002 + qerr) * 1.000004);
  h.eB = round_up_f32(((double)a.err_coef * qs + 1.001 * qerr) * 1.000004 + 1e-37);
  return h;
}

// ---- the listed rows in 8 bits: wave b settles segment b, which it has just written -------------------------------------------
// screen_kernel's 8-bit score and interval (the device functions of screen_core.h, its lane layout with G lanes per 8-bit row,
// so kacc holds as derived there), top-2 / U3 / L tracks, and partial b of scr_partials in screen_kernel's format.
template <int G, int CH, int UR>
__device__ __forceinline__ void settle8(const Front4Args& a, const int* seg, int b, int cnt, float qscale) {
  constexpr int RPW = 64 / G;
  const int lane = threadIdx.x & 63;
  const int sub = lane % G, rsub = lane / G;
  const bool ovf = cnt > a.seg_cap;

  Track<float> tr;
  tr.U1 = tr.U2 = tr.U3 = tr.L = -INFINITY;
  tr.i1 = tr.i2 = 0x7fffffff;
  if (!ovf && cnt > 0) {
    Q16 q0[CH];
    int voff[CH];
    float qs0 = 0.0f;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const int v = c * G + sub;
      const bool ok = v < a.ldv8;
      voff[c] = ok ? v : 0;
      q0[c] = load_q16(a.q, v, a.d, ok, qs0);
    }
    const float off0 = -128.0f * qs0;
    // (the segment is in increasing row order and a lane group walks it in order: track_update keeps the lowest index on ties)
    int nxt[UR];
#pragma unroll
    for (int u = 0; u < UR; ++u) { const int kk = u * RPW + rsub; nxt[u] = kk < cnt ? seg[kk] : -1; }
    for (int k0 = 0; k0 < cnt; k0 += RPW * UR) {
      int row[UR];
      uint4 x[UR][CH];
      float2 sbv[UR];
#pragma unroll
      for (int u = 0; u < UR; ++u) row[u] = nxt[u];
#pragma unroll
      for (int u = 0; u < UR; ++u) { const int kk = k0 + RPW * UR + u * RPW + rsub; nxt[u] = kk < cnt ? seg[kk] : -1; }   // a trip ahead
#pragma unroll
      for (int u = 0; u < UR; ++u) {
        const int64_t rc = row[u] < 0 ? 0 : row[u];
        const uint4* p = (const uint4*)a.Aq + rc * a.ldv8;
#pragma unroll
        for (int c = 0; c < CH; ++c) x[u][c] = stream_load(p + voff[c]);
        sbv[u] = a.sb8[rc];
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int u = 0; u < UR; ++u) {
        float t0 = off0;
#pragma unroll
        for (int c = 0; c < CH; ++c) t0 = dot16(x[u][c], q0[c], t0);
        float s0 = group_allsum<float, G>(t0);
        s0 *= sbv[u].x;
        float U, L;
        screen_interval(s0, sbv[u].x, sbv[u].y, a.kacc, a.err_coef, qscale, U, L);
        if (row[u] < 0) { U = -INFINITY; L = -INFINITY; }
        track_update<float>(tr, U, L, row[u] < 0 ? 0x7fffffff : row[u]);
      }
    }
#pragma unroll
    for (int off = G; off < 64; off <<= 1) tr = merge<float>(tr, shfl_track<float>(tr, off));
  }
  if (lane == 0) {
    if (ovf) {   // a full segment: unseen rows above anything -- refine_kernel reports the overflow it already knows
      tr.U1 = tr.U2 = tr.L = -INFINITY; tr.U3 = INFINITY; tr.i1 = tr.i2 = 0x7fffffff;
    }
    a.out.U1[b] = (double)tr.U1; a.out.U2[b] = (double)tr.U2; a.out.U3[b] = (double)tr.U3; a.out.L[b] = (double)tr.L;
    a.out.i1[b] = tr.i1; a.out.i2[b] = tr.i2;
  }
}

template <int G, int CH, int UR, int G8, int CH8, int UR8>
__global__ __launch_bounds__(BCX_SCAN_THREADS) void front4_kernel(Front4Args a) {
  // lane l's sentinel row (l mod 16 of this wave's 16) is requested together with the flag -- one round trip, not two; the
  // empty statement keeps the load in front of the branch
  int myrow = a.sent[(threadIdx.x >> 6) * BCX_S4_SPW + (threadIdx.x & (BCX_S4_SPW - 1))];
  const float qscale = (float)a.st->qscale;
  const int active = a.st->active;
  asm volatile("" : "+v"(myrow));
  if (!active) return;
  if (!(myrow >= 0 && (int64_t)myrow < a.n)) myrow = -1;
  const float2 mysb = a.sb8[myrow < 0 ? 0 : myrow];
  __shared__ double scratch[BCX_SCRATCH];
  __shared__ unsigned planes[3 * BCX_S4_MAX_NW4];
  __shared__ int lseg[BCX_SCREEN_WAVES][BCX_S4_SEG_CAP];   // the wave's list once more, for its own second stage
  constexpr int RPW = 64 / G;
  constexpr int WAVES = BCX_SCREEN_WAVES;
  constexpr int RPB = WAVES * RPW * UR;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int sub = lane % G, rsub = lane / G;
  int voff[CH];
  bool vok[CH];
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    const int v = c * G + sub;
    vok[c] = v < a.ldv;
    voff[c] = vok[c] ? v : 0;     // clamp: the load stays inside the row, the zero query kills the product
  }
  const int b = blockIdx.x * WAVES + wave;
  int* seg = a.list + (size_t)b * BCX_S4_SEG_CAP;
  int cnt = 0;
  const int64_t n = a.n;
  const int64_t stride = (int64_t)gridDim.x * RPB;
  uint4 x[UR][CH];
  float2 sbv[UR];
  auto load_trip = [&](int64_t r0) {
#pragma unroll
    for (int u = 0; u < UR; ++u) {
      const int64_t rw = r0 + (int64_t)(u * WAVES + wave) * RPW + rsub;
      const int64_t rc = rw < n ? rw : n - 1;
      const uint4* p = a.A4 + rc * a.ldv;
#pragma unroll
      for (int c = 0; c < CH; ++c) x[u][c] = stream_load(p + voff[c]);
      sbv[u] = a.sb[rc];
    }
  };
  // the first trip's loads depend on nothing the head computes: they are in flight while it runs (the launch has a
  // workgroup only where it has rows, and a clamped load is inside the array whatever r0 is)
  int64_t r0 = (int64_t)blockIdx.x * RPB;
  load_trip(r0);
  __builtin_amdgcn_sched_barrier(0);
  const Front4Head h = front4_head(a, myrow, mysb, qscale, planes, scratch);
  int qp[CH][4][3];
#pragma unroll
  for (int c = 0; c < CH; ++c)
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
      for (int p = 0; p < 3; ++p) qp[c][k][p] = vok[c] ? (int)planes[p * a.nw4 + 4 * voff[c] + k] : 0;
  for (;;) {
    __builtin_amdgcn_sched_barrier(0);   // all loads of the trip in flight before the first use (see scan_kernel)
#pragma unroll
    for (int u = 0; u < UR; ++u) {
      int a0 = 0, a1 = 0, a2 = 0;
#pragma unroll
      for (int c = 0; c < CH; ++c) {
        const unsigned xs[4] = {x[u][c].x, x[u][c].y, x[u][c].z, x[u][c].w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int cw = (int)(xs[k] ^ 0x88888888u);   // c + 8 -> two's-complement nibble
          a0 = __builtin_amdgcn_sdot8(cw, qp[c][k][0], a0, false);
          a1 = __builtin_amdgcn_sdot8(cw, qp[c][k][1], a1, false);
          a2 = __builtin_amdgcn_sdot8(cw, qp[c][k][2], a2, false);
        }
      }
      const int tot = group_allsum_i32<G>((a2 * 16 + a1) * 16 + a0);
      const float s4 = (sbv[u].x * h.qstep) * (float)tot;
      const float e4 = fmaf(sbv[u].y, h.eA, h.eB) + fabsf(s4) * 5e-7f;
      const float U4 = s4 + e4;
      const int64_t rw = r0 + (int64_t)(u * WAVES + wave) * RPW + rsub;
      const bool want = rw < n && sub == 0 && !(U4 < h.Lg);   // (a NaN bound lists the row)
      const unsigned long long bal = __ballot(want);
      if (bal) {                                             // (wave-uniform)
        const int pos = cnt + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(bal >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bal, 0u));
        if (want && pos < a.seg_cap) { seg[pos] = (int)rw; lseg[wave][pos] = (int)rw; }
        cnt += __popcll(bal);
      }
    }
    r0 += stride;
    if (!(r0 < n)) break;
    load_trip(r0);
  }
  if (lane == 0) a.counts[b] = cnt;
  // The wave settles its own list in the same launch, from the copy in LDS: the gathers of a wave that has finished its
  // stream run beside the streams of the others.
  settle8<G8, CH8, UR8>(a, lseg[wave], b, cnt, qscale);
}

// ---- quantiser: one wave per row; a lane owns dwords of 8 consecutive elements ---------------------------------------------------
template <bool F16>
__global__ __launch_bounds__(256) void quantise4_kernel(const void* An, int ld, int d, int nw4, int64_t n, unsigned* A4, float2* sb) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n) return;
  auto elem = [&](int j) -> float {
    if (F16) return __half2float(((const __half*)An)[row * (int64_t)ld + j]);
    return ((const float*)An)[row * (int64_t)ld + j];
  };
  float m = 0.0f;
  for (int j = lane; j < d; j += 64) m = fmaxf(m, fabsf(elem(j)));
  m = (float)wave_allmax((double)m);
  float sc = (float)((double)m * BCX_S4_CLIP / 7.0);
  if (!(sc >= FLT_MIN)) sc = FLT_MIN;
  const double dsc = (double)sc;
  double r2 = 0.0;
  for (int w = lane; w < nw4; w += 64) {
    unsigned word = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int j = 8 * w + k;
      int code = 0;
      if (j < d) {
        const double v = (double)elem(j);
        double c = rint(v / dsc);
        c = c > 7.0 ? 7.0 : (c < -7.0 ? -7.0 : c);
        if (c != c) c = 0.0;
        code = (int)c;
        const double r = v - c * dsc;     // (clipped elements: the whole excess is in r)
        r2 = fma(r, r, r2);
      }
      word |= (unsigned)(code + 8) << (4 * k);
    }
    A4[row * (int64_t)nw4 + w] = word;
  }
  r2 = wave_allsum(r2);
  if (lane == 0) {
    const double b = sqrt(r2) * (1.0 + 9.5367431640625e-07);
    float bf = (float)b;
    if ((double)bf < b) bf = nextafterf(bf, INFINITY);
    if (!(bf == bf)) bf = INFINITY;      // NaN in the row: it is always listed
    sb[row] = make_float2(sc, bf);
  }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------
bool bcx_screen4_on(const bcx_solver* s) {
  return s->s4_enabled && !s->s4_dropped && bcx_screen_on(s) && s->cfg.alg != BCX_ALG_GIGA && s->cfg.world_size == 1;
}

// Build (or rebuild after a reload) the 4-bit shadow, after bcx_screen_build.  No room: the solver stays on the 8-bit tier.
int bcx_screen4_build(bcx_solver* s) {
  if (s->s4_valid || !bcx_screen4_on(s) || !s->scr_valid) return BCX_OK;
  const int d = s->cfg.d;
  const int64_t n = s->cfg.n_local;
  s->ld4 = (d + 31) / 32 * 16;
  const int nw4 = s->ld4 / 4;
  if (s->s4_sb.count() < (size_t)n || !s->A4) {
    auto drop = [&]() { s->A4.reset(); s->s4_sb.reset(); s->s4_list.reset(); s->s4_counts.reset(); s->s4_sent.reset(); };
    drop();      // all go before any is asked for again
    if (s->A4.alloc((size_t)n * s->ld4, false) || s->s4_sb.alloc((size_t)n, false) ||
        s->s4_list.alloc((size_t)BCX_MAX_PARTIALS * BCX_S4_SEG_CAP, false) || s->s4_counts.alloc((size_t)BCX_MAX_PARTIALS, false) ||
        s->s4_sent.alloc((size_t)BCX_S4_SENTINELS, false)) {
      (void)hipGetLastError();
      drop();
      s->s4_dropped = 2;
      return BCX_OK;
    }
    // no sentinels yet (-1 each); s4_warm below keeps the front pass away until a refine_kernel has written them
    BCX_HIP(hipMemsetAsync(s->s4_sent, 0xff, (size_t)BCX_S4_SENTINELS * 4, s->stream));
  }
  const unsigned grid = (unsigned)((n + 3) / 4);
  if (s->cfg.store_dtype == BCX_F16)
    hipLaunchKernelGGL((quantise4_kernel<true>), dim3(grid), dim3(256), 0, s->stream, s->An, s->ld, d, nw4, n, (unsigned*)s->A4.get(), s->s4_sb.get());
  else
    hipLaunchKernelGGL((quantise4_kernel<false>), dim3(grid), dim3(256), 0, s->stream, s->An, s->ld, d, nw4, n, (unsigned*)s->A4.get(), s->s4_sb.get());
  BCX_HIP(hipGetLastError());
  s->s4_valid = true;
  s->s4_warm = 2;          // new rows: the sentinels the last refine left name rows of the old ones
  return BCX_OK;
}

// The pairs of 4-bit (G, CH) and 8-bit (G8, CH8) lane geometry that one d can produce (ld4 = ceil(d / 32) pieces, ld8 =
// ceil(d / 16)); UR is 8 loads in flight where a lane has one piece, UR8 the rows of a second-stage trip per lane group (16 / CH8).
static int launch_front4(bcx_solver* s, const Front4Args& a, int G, int CH, int G8, int CH8, int grid) {
  dim3 g(grid), b(BCX_SCAN_THREADS);
#define L(GG, CC, UU, G8_, C8_, U8_)                                                                   \
  if (G == GG && CH == CC && G8 == G8_ && CH8 == C8_) {                                                \
    hipLaunchKernelGGL((front4_kernel<GG, CC, UU, G8_, C8_, U8_>), g, b, 0, s->stream, a);             \
    return BCX_OK;                                                                                     \
  }
  L(1, 1, 8, 1, 1, 16) L(1, 1, 8, 2, 1, 16) L(2, 1, 8, 4, 1, 16) L(4, 1, 8, 8, 1, 16) L(8, 1, 8, 16, 1, 16)
  L(16, 1, 8, 32, 1, 16) L(32, 1, 8, 64, 1, 16) L(64, 1, 8, 64, 2, 8) L(64, 2, 4, 64, 4, 4)
#undef L
  s->err = "front4: unsupported row length";
  return BCX_ERR_ARG;
}

// The launch plan of one front pass: the kernel's arguments, the pair of lane geometries and the grid.  One text for the
// iteration (bcx_launch_screen4) and for the diagnostic probe (bcx_launch_front4_probe).
struct Front4Plan { Front4Args f; int G, CH, G8, CH8, grid, n_in; };

static int front4_plan(bcx_solver* s, Front4Plan* p) {
  const int d = s->cfg.d;
  const int64_t n = s->cfg.n_local;
  const int nw4 = s->ld4 / 4;
  if (nw4 > BCX_S4_MAX_NW4) { s->err = "front4: unsupported row length"; return BCX_ERR_ARG; }
  ScanArgs sa;
  ScanPlan sp;
  int rc = bcx_scan_plan(s, 0, &sa, &sp);
  if (rc != BCX_OK) return rc;
  const int ldv8 = s->ld8 / 16;
  const int G8 = screen_group(ldv8), CH8 = screen_chunks(ldv8, G8);
  const float kacc = screen_kacc(G8, CH8, d);

  Front4Args& f = p->f;
  f.A4 = (const uint4*)s->A4.get(); f.sb = s->s4_sb; f.q = (const float*)s->qst.get(); f.sent = s->s4_sent;
  f.Aq = (const unsigned char*)s->Aq.get(); f.sb8 = s->scr_sb; f.st = s->st;
  f.list = s->s4_list; f.counts = s->s4_counts;
  f.n = n; f.ldv = s->ld4 / 16; f.nw4 = nw4; f.seg_cap = s->s4_seg_cap;
  f.ld8 = s->ld8; f.d = d; f.kacc = kacc; f.err_coef = sa.err_coef;
  const int G = screen_group(f.ldv), CH = screen_chunks(f.ldv, G);
  // eight 16-byte loads in flight per lane and 512 workgroups: at c4 2167 it/s against 2068 with four loads, 1821 with
  // eight loads on 256 workgroups and 1336 with four on 256 (profiles/screen4_ab.txt); every wave owns one list segment and
  // one of the BCX_MAX_PARTIALS partials.  No workgroup without rows: grid <= ceil(n / rpb).
  const int ur = CH == 1 ? 8 : 4;
  const int rpb = BCX_SCREEN_WAVES * (64 / G) * ur;
  const int64_t want = (n + rpb - 1) / rpb;
  int cap = 512;
  if (cap > BCX_MAX_PARTIALS / BCX_SCREEN_WAVES) cap = BCX_MAX_PARTIALS / BCX_SCREEN_WAVES;
  const int grid = (int)(want < 1 ? 1 : (want > cap ? cap : want));

  const int n_in = grid * BCX_SCREEN_WAVES;
  f.out = partial_view(s->scr_partials, n_in); f.ldv8 = ldv8;
  p->G = G; p->CH = CH; p->G8 = G8; p->CH8 = CH8; p->grid = grid; p->n_in = n_in;
  return BCX_OK;
}

// One 4-bit iteration's front: the front pass (which computes its own threshold and settles its list), then refine.  Afterwards s->partials /
// s->n_partials are what bcx_launch_screen leaves.  The caller (api.hip) has made sure that the refine kernel of the tier
// iteration enqueued just before has left sentinel rows.
int bcx_launch_screen4(bcx_solver* s) {
  Front4Plan p;
  int rc = front4_plan(s, &p);
  if (rc != BCX_OK) return rc;
  if ((rc = launch_front4(s, p.f, p.G, p.CH, p.G8, p.CH8, p.grid))) return rc;
  BCX_HIP(hipGetLastError());
  s->scr_n_in = p.n_in;
  return bcx_launch_refine(s, p.n_in, true);
}

// One launch of front4_kernel and nothing else (bcx_screen4_probe, api.hip): the same plan, no refine, no counters.  The
// caller has set the query, the state and the sentinels; *n_waves is the number of list segments / partials it wrote.
int bcx_launch_front4_probe(bcx_solver* s, int* n_waves) {
  Front4Plan p;
  int rc = front4_plan(s, &p);
  if (rc != BCX_OK) return rc;
  if ((rc = launch_front4(s, p.f, p.G, p.CH, p.G8, p.CH8, p.grid))) return rc;
  BCX_HIP(hipGetLastError());
  *n_waves = p.n_in;
  return BCX_OK;
}
