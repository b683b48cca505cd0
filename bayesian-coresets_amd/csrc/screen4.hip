// screen4.hip -- a 4-bit front pass in front of the 8-bit screening tier (single-query algorithms: FW, OMP; one shard).
//
// The 8-bit tier (screen8.hip) streams one byte per element every greedy iteration and runs at the HBM rate: the step is the
// bytes of its shadow.  This file keeps a second, coarser shadow of half a byte per element and streams THAT; the 8-bit
// shadow is then read only for the rows the coarse pass cannot exclude.  What makes four bits enough is that the cut-off is
// known BEFORE the pass: the lower bound of any row is a lower bound of the maximum, so a handful of rows that led the
// previous iteration ("sentinels"), scored in 8 bits against the new query, give a threshold Lg, and a row whose 4-bit UPPER
// bound is below Lg is out -- only the one-sided 4-bit error enters.  A poor threshold lists more rows; it never changes
// the result.  Kernels of one 4-bit iteration, in stream order:
//
//   thresh4_kernel : one workgroup.  (a) The fp32 query q~ becomes integers x_j = rint(q~_j / qstep) in [-1911, 1911],
//                    qstep = max|q~| / 1911, written as three planes of signed nibbles x = 256 h2 + 16 h1 + l, each digit
//                    in [-8, 7], eight elements per dword -- the operand format of v_dot8_i32_i4.  qerr is an fp32 round-up
//                    of || q~ - x qstep ||_2 summed in fp64.  (b) The sentinels: the partials the previous tier iteration
//                    left in scr_partials name two rows per wave with their 8-bit upper bounds; each of the 16 waves here
//                    owns an interleaved sixteenth of those candidates and takes its 4 largest (64 rows; among them the
//                    4 largest overall).  (c) Each sentinel is scored from the 8-bit shadow against the new query (products
//                    exact, sum in fp64) and gets screen_interval's lower bound, the one screen_kernel would give it;
//                    Lg is their maximum.  Lg, qstep and the two coefficients of e4 go to one 16-byte head that every
//                    consumer reads: there is one Lg.
//   front4_kernel  : screen_kernel's streaming structure (16-byte non-temporal loads, G lanes per row, <= 512 workgroups)
//                    over the 4-bit codes, without tracks.  A dword holds eight codes c + 8, element 8 w + k in bits 4k..4k+3;
//                    xor 0x88888888 turns them into two's-complement nibbles, three v_dot8_i32_i4 against the query planes
//                    give exact integer sums (|sum| <= 4096 * 7 * 1911 < 2^26), 4 instructions per 8 elements.
//                      score4 = scale4 * qstep * sum_j c_j x_j ,   U4 = score4 + e4
//                    A row with not (U4 < Lg) is appended to the wave's own segment of the list buffer (BCX_S4_SEG_CAP
//                    entries; ballot + prefix count, the fill count stays in a register, no atomics).  A wave that wanted
//                    to list more says so by its count.
//   second8_kernel : wave w reads segment w and gives the listed rows screen_kernel's 8-bit score and interval (the device
//                    functions of screen_core.h, same lane layout, so kacc holds as derived there), tracks top-2 / U3 / L
//                    and writes partial w of scr_partials in screen_kernel's format.  A wave whose segment overflowed writes
//                    the partial that makes refine_kernel report an overflow.  refine_kernel, resolve_core, the fp64
//                    re-score and the tail follow unchanged, and the same partials name the next iteration's sentinels.
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
#define BCX_THRESH_THREADS 1024

struct Front4Head { float Lg, qstep, eA, eB; };

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

// ---- threshold ------------------------------------------------------------------------------------------------------------
struct Thresh4Args {
  PartialView in;       // the previous tier iteration's per-wave partials
  int n_in;
  const unsigned char* Aq;   // 8-bit shadow
  const float2* sb;
  const float* q;
  const DevState* st;
  unsigned long long* stat;
  unsigned* head;       // Front4Head, then 3 planes of nw4 dwords
  const int* counts;    // the previous 4-bit iteration's list counts, n_seg of them (booked here: see SCR4_PENDING)
  int n_seg;
  int seg_cap;          // entries of a segment in use (BCX_S4_SEG_CAP; less under the dev switch)
  int64_t n;
  int ld8, d, nw4;
  float kacc, err_coef; // of the 8-bit tier (screen_interval)
};

__global__ __launch_bounds__(BCX_THRESH_THREADS) void thresh4_kernel(Thresh4Args a) {
  if (!a.st->active) return;
  __shared__ double scratch[BCX_SCRATCH];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  constexpr int NW = BCX_THRESH_THREADS / 64;
  // the candidates' loads go first: nothing below depends on the query until the rows are scored
  constexpr int PT = 2 * BCX_MAX_PARTIALS / BCX_THRESH_THREADS;
  double cu[PT];
  int ci[PT];
#pragma unroll
  for (int t = 0; t < PT; ++t) {
    const int c = wave + NW * (lane + 64 * t);
    const int p = c >> 1;
    const bool ok = p < a.n_in;
    const double u = ok ? ((c & 1) ? a.in.U2[p] : a.in.U1[p]) : -INFINITY;
    const int i = ok ? ((c & 1) ? a.in.i2[p] : a.in.i1[p]) : -1;
    const bool use = u > -INFINITY && i >= 0 && (int64_t)i < a.n;   // (false for NaN)
    cu[t] = use ? u : -INFINITY; ci[t] = use ? i : -1;
  }
  // (a) the query in three nibble planes
  double m = 0.0;
  for (int j = tid; j < a.d; j += BCX_THRESH_THREADS) {
    const double v = fabs((double)a.q[j]);
    m = fmax(m, v == v ? v : INFINITY);
  }
  m = block_allmax(m, scratch);
  float step = (float)(m / BCX_S4_QMAX);
  const bool qok = m < INFINITY && step >= FLT_MIN;   // else: nothing is excluded this iteration (Lg = -inf)
  if (!qok) step = 0.0f;
  // (b) sentinels: this wave's 4 largest upper bounds among its sixteenth of the 2 n_in candidates
  constexpr int SPW = BCX_S4_SENTINELS / NW;
  int rows[SPW];
#pragma unroll
  for (int r = 0; r < SPW; ++r) {
    double best = -INFINITY;
    int bt = -1, bi = -1;
#pragma unroll
    for (int t = 0; t < PT; ++t) if (cu[t] > best) { best = cu[t]; bt = t; bi = ci[t]; }
    const double wm = wave_allmax(best);
    const unsigned long long bal = __ballot(bt >= 0 && best == wm);
    const int src = bal ? __ffsll((long long)bal) - 1 : 0;
    const int row = __shfl(bi, src, BCX_WAVE);
    rows[r] = bal ? row : -1;                 // (wave-uniform) -1: no candidates left
#pragma unroll
    for (int t = 0; t < PT; ++t) if (bal && lane == src && t == bt) cu[t] = -INFINITY;
  }
  // (c) their 8-bit scores against the new query: the four rows' loads of a trip are independent
  double acc[SPW];
#pragma unroll
  for (int r = 0; r < SPW; ++r) acc[r] = 0.0;
  const int nw8 = a.ld8 / 4;
  const unsigned* A8 = (const unsigned*)a.Aq;
  for (int w = lane; w < nw8; w += 64) {
    unsigned cw[SPW];
#pragma unroll
    for (int r = 0; r < SPW; ++r) cw[r] = A8[(int64_t)(rows[r] < 0 ? 0 : rows[r]) * nw8 + w];
    double qv[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) { const int j = 4 * w + k; const float t = a.q[j < a.d ? j : 0]; qv[k] = j < a.d ? (double)t : 0.0; }
#pragma unroll
    for (int r = 0; r < SPW; ++r)
#pragma unroll
      for (int k = 0; k < 4; ++k) acc[r] = fma((double)((int)((cw[r] >> (8 * k)) & 0xffu) - 128), qv[k], acc[r]);
  }
  // [0] the query's squared rounding error; [1] rows listed and [2] full segments of the previous 4-bit iteration
  double err2[3] = {0.0, 0.0, 0.0};
  if (a.stat[SCR4_PENDING])
    for (int p = tid; p < a.n_seg; p += BCX_THRESH_THREADS) {
      const int c = a.counts[p];
      err2[1] += (double)(c > a.seg_cap ? a.seg_cap : c);
      err2[2] += c > a.seg_cap ? 1.0 : 0.0;
    }
  for (int w = tid; w < a.nw4; w += BCX_THRESH_THREADS) {
    unsigned p0 = 0, p1 = 0, p2 = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int j = 8 * w + k;
      int x = 0;
      if (j < a.d && qok) {
        const double v = (double)a.q[j];
        double c = rint(v / (double)step);
        c = c > BCX_S4_QMAX ? BCX_S4_QMAX : (c < -BCX_S4_QMAX ? -BCX_S4_QMAX : c);
        x = (int)c;
        const double r = v - c * (double)step;
        err2[0] = fma(r, r, err2[0]);
      }
      const int l = ((x + 8) & 15) - 8;
      const int x1 = (x - l) >> 4;
      const int h1 = ((x1 + 8) & 15) - 8;
      const int h2 = (x1 - h1) >> 4;
      p0 |= (unsigned)(l & 15) << (4 * k); p1 |= (unsigned)(h1 & 15) << (4 * k); p2 |= (unsigned)(h2 & 15) << (4 * k);
    }
    a.head[4 + w] = p0; a.head[4 + a.nw4 + w] = p1; a.head[4 + 2 * a.nw4 + w] = p2;
  }
  block_allsum<3>(err2, scratch);
  const double qerr = sqrt(err2[0]) * (1.0 + 9.5367431640625e-07);
  const float qscale = (float)a.st->qscale;
  float lmax = -INFINITY;
#pragma unroll
  for (int r = 0; r < SPW; ++r) {
    const double tot = wave_allsum(acc[r]);
    const float2 sb = a.sb[rows[r] < 0 ? 0 : rows[r]];
    const float s0 = (float)((double)sb.x * tot);   // one rounding, inside the 2e-7 |s| of screen_interval
    float U, L;
    screen_interval(s0, sb.x, sb.y, a.kacc, a.err_coef, qscale, U, L);
    if (rows[r] >= 0) lmax = fmaxf(lmax, L);        // (a NaN bound is no bound: fmaxf drops it)
  }
  const double lg = block_allmax((double)lmax, scratch);
  if (tid == 0) {
    const double qs = (double)qscale;
    Front4Head h;
    h.Lg = qok ? (float)lg : -INFINITY;
    h.qstep = step;
    h.eA = round_up_f32((qs * 1.000002 + qerr) * 1.000004);
    h.eB = round_up_f32(((double)a.err_coef * qs + 1.001 * qerr) * 1.000004 + 1e-37);
    *(Front4Head*)a.head = h;
    a.stat[SCR4_LAST] = a.stat[SCR_ITERS] + 1ull;
    a.stat[SCR4_ITERS] += 1ull;
    a.stat[SCR4_LISTED] += (unsigned long long)err2[1];
    a.stat[SCR4_OVERFLOWS] += (unsigned long long)err2[2];
    a.stat[SCR4_PENDING] = 1ull;
  }
}

// ---- front pass -------------------------------------------------------------------------------------------------------------
struct Front4Args {
  const uint4* A4;      // n x ldv pieces of 32 codes
  const float2* sb;     // per row: (scale4, bound4)
  const unsigned* head; // thresh4_kernel's output
  const DevState* st;
  int* list;            // one segment of BCX_S4_SEG_CAP entries per wave, of which seg_cap are in use
  int* counts;          // rows the wave wanted to list
  int64_t n;
  int ldv, nw4, seg_cap;
};

template <int G, int CH, int UR>
__global__ __launch_bounds__(BCX_SCAN_THREADS) void front4_kernel(Front4Args a) {
  if (!a.st->active) return;
  constexpr int RPW = 64 / G;
  constexpr int WAVES = BCX_SCREEN_WAVES;
  constexpr int RPB = WAVES * RPW * UR;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int sub = lane % G, rsub = lane / G;
  const Front4Head h = *(const Front4Head*)a.head;
  const unsigned* planes = a.head + 4;
  int qp[CH][4][3];
  int voff[CH];
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    const int v = c * G + sub;
    const bool ok = v < a.ldv;
    voff[c] = ok ? v : 0;     // clamp: the load stays inside the row, the zero query kills the product
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
      for (int p = 0; p < 3; ++p) {
        const unsigned w = planes[p * a.nw4 + 4 * voff[c] + k];
        qp[c][k][p] = ok ? (int)w : 0;
      }
  }
  const int b = blockIdx.x * WAVES + wave;
  int* seg = a.list + (size_t)b * BCX_S4_SEG_CAP;
  int cnt = 0;
  const int64_t n = a.n;
  const int64_t stride = (int64_t)gridDim.x * RPB;
  for (int64_t r0 = (int64_t)blockIdx.x * RPB; r0 < n; r0 += stride) {
    uint4 x[UR][CH];
    float2 sbv[UR];
#pragma unroll
    for (int u = 0; u < UR; ++u) {
      const int64_t rw = r0 + (int64_t)(u * WAVES + wave) * RPW + rsub;
      const int64_t rc = rw < n ? rw : n - 1;
      const uint4* p = a.A4 + rc * a.ldv;
#pragma unroll
      for (int c = 0; c < CH; ++c) x[u][c] = stream_load(p + voff[c]);
      sbv[u] = a.sb[rc];
    }
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
        if (want && pos < a.seg_cap) seg[pos] = (int)rw;
        cnt += __popcll(bal);
      }
    }
  }
  if (lane == 0) a.counts[b] = cnt;
}

// ---- second stage: the listed rows in 8 bits ----------------------------------------------------------------------------------
struct Second8Args {
  const uint4* Aq;
  const float2* sb;
  const float* q;
  const DevState* st;
  const int* list;
  const int* counts;
  PartialView out;      // one partial per wave, screen_kernel's format
  int ldv, d, seg_cap;
  float kacc, err_coef;
};

template <int G, int CH, int UR>
__global__ __launch_bounds__(BCX_SCAN_THREADS) void second8_kernel(Second8Args a) {
  if (!a.st->active) return;
  constexpr int RPW = 64 / G;
  constexpr int WAVES = BCX_SCREEN_WAVES;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int sub = lane % G, rsub = lane / G;
  const int b = blockIdx.x * WAVES + wave;
  const int cnt = __builtin_amdgcn_readfirstlane(a.counts[b]);
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
      const bool ok = v < a.ldv;
      voff[c] = ok ? v : 0;
      q0[c] = load_q16(a.q, v, a.d, ok, qs0);
    }
    const float off0 = -128.0f * qs0;
    const float qscale = (float)a.st->qscale;
    const int* seg = a.list + (size_t)b * BCX_S4_SEG_CAP;
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
        const uint4* p = a.Aq + rc * a.ldv;
#pragma unroll
        for (int c = 0; c < CH; ++c) x[u][c] = stream_load(p + voff[c]);
        sbv[u] = a.sb[rc];
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

static size_t head_bytes(int nw4) { return sizeof(Front4Head) + (size_t)3 * nw4 * 4; }

// Build (or rebuild after a reload) the 4-bit shadow, after bcx_screen_build.  No room: the solver stays on the 8-bit tier.
int bcx_screen4_build(bcx_solver* s) {
  if (s->s4_valid || !bcx_screen4_on(s) || !s->scr_valid) return BCX_OK;
  const int d = s->cfg.d;
  const int64_t n = s->cfg.n_local;
  s->ld4 = (d + 31) / 32 * 16;
  const int nw4 = s->ld4 / 4;
  if (s->s4_cap_rows < n || !s->A4) {
    void** all[] = {&s->A4, &s->s4_sb, &s->s4_list, &s->s4_counts, &s->s4_head};
    for (void** p : all) { if (*p) (void)hipFree(*p); *p = nullptr; }
    s->s4_cap_rows = 0;
    hipError_t e = hipMalloc(&s->A4, (size_t)n * s->ld4);
    if (e == hipSuccess) e = hipMalloc(&s->s4_sb, (size_t)n * 8);
    if (e == hipSuccess) e = hipMalloc(&s->s4_list, (size_t)BCX_MAX_PARTIALS * BCX_S4_SEG_CAP * 4);
    if (e == hipSuccess) e = hipMalloc(&s->s4_counts, (size_t)BCX_MAX_PARTIALS * 4);
    if (e == hipSuccess) e = hipMalloc(&s->s4_head, head_bytes(nw4));
    if (e != hipSuccess) {
      (void)hipGetLastError();
      for (void** p : all) { if (*p) (void)hipFree(*p); *p = nullptr; }
      s->s4_dropped = 2;
      return BCX_OK;
    }
    s->s4_cap_rows = n;
    // new buffers: no counts of an earlier front pass are waiting to be booked
    BCX_HIP(hipMemsetAsync(s->s4_counts, 0, (size_t)BCX_MAX_PARTIALS * 4, s->stream));
    BCX_HIP(hipMemsetAsync(s->scr_stat + SCR4_PENDING, 0, sizeof(unsigned long long), s->stream));
    s->s4_n_seg = 0;
  }
  const unsigned grid = (unsigned)((n + 3) / 4);
  if (s->cfg.store_dtype == BCX_F16)
    hipLaunchKernelGGL((quantise4_kernel<true>), dim3(grid), dim3(256), 0, s->stream, s->An, s->ld, d, nw4, n, (unsigned*)s->A4, (float2*)s->s4_sb);
  else
    hipLaunchKernelGGL((quantise4_kernel<false>), dim3(grid), dim3(256), 0, s->stream, s->An, s->ld, d, nw4, n, (unsigned*)s->A4, (float2*)s->s4_sb);
  BCX_HIP(hipGetLastError());
  s->s4_valid = true;
  s->s4_warm = 2;          // new rows: whatever scr_partials hold names rows of the old ones
  return BCX_OK;
}

static int launch_front4(bcx_solver* s, const Front4Args& a, int G, int CH, int UR, int grid) {
  dim3 g(grid), b(BCX_SCAN_THREADS);
#define L(GG, CC, UU)                                                                  \
  if (G == GG && CH == CC && UR == UU) {                                               \
    hipLaunchKernelGGL((front4_kernel<GG, CC, UU>), g, b, 0, s->stream, a);            \
    return BCX_OK;                                                                     \
  }
  L(1, 1, 4) L(2, 1, 4) L(4, 1, 4) L(8, 1, 4) L(16, 1, 4) L(32, 1, 4) L(64, 1, 4) L(64, 2, 4)
  L(1, 1, 8) L(2, 1, 8) L(4, 1, 8) L(8, 1, 8) L(16, 1, 8) L(32, 1, 8) L(64, 1, 8)
#undef L
  s->err = "front4: unsupported row length";
  return BCX_ERR_ARG;
}

static int launch_second8(bcx_solver* s, const Second8Args& a, int G, int CH, int grid) {
  dim3 g(grid), b(BCX_SCAN_THREADS);
#define L(GG, CC, UU)                                                                  \
  if (G == GG && CH == CC) {                                                           \
    hipLaunchKernelGGL((second8_kernel<GG, CC, UU>), g, b, 0, s->stream, a);           \
    return BCX_OK;                                                                     \
  }
  L(1, 1, 16) L(2, 1, 16) L(4, 1, 16) L(8, 1, 16) L(16, 1, 16) L(32, 1, 16) L(64, 1, 16) L(64, 2, 8) L(64, 4, 4)
#undef L
  s->err = "second8: unsupported row length";
  return BCX_ERR_ARG;
}

// One 4-bit iteration's front: threshold, front pass, second stage, refine.  Afterwards s->partials / s->n_partials are what
// bcx_launch_screen leaves.  The caller (api.hip) has made sure that scr_partials hold a tier iteration's partials.
int bcx_launch_screen4(bcx_solver* s) {
  const int d = s->cfg.d;
  const int64_t n = s->cfg.n_local;
  const int nw4 = s->ld4 / 4;
  ScanArgs sa;
  ScanPlan sp;
  int rc = bcx_scan_plan(s, 0, &sa, &sp);
  if (rc != BCX_OK) return rc;
  const int ldv8 = s->ld8 / 16;
  const int G8 = screen_group(ldv8), CH8 = screen_chunks(ldv8, G8);
  const float kacc = screen_kacc(G8, CH8, d);

  Thresh4Args t;
  t.in = partial_view(s->scr_partials, s->scr_n_in); t.n_in = s->scr_n_in;
  t.Aq = (const unsigned char*)s->Aq; t.sb = (const float2*)s->scr_sb; t.q = (const float*)s->qst;
  t.st = s->st; t.stat = s->scr_stat; t.head = (unsigned*)s->s4_head;
  t.n = n; t.ld8 = s->ld8; t.d = d; t.nw4 = nw4;
  t.kacc = kacc; t.err_coef = sa.err_coef;

  Front4Args f;
  f.A4 = (const uint4*)s->A4; f.sb = (const float2*)s->s4_sb; f.head = (const unsigned*)s->s4_head; f.st = s->st;
  f.list = (int*)s->s4_list; f.counts = (int*)s->s4_counts;
  f.n = n; f.ldv = s->ld4 / 16; f.nw4 = nw4;
  const int G = screen_group(f.ldv), CH = screen_chunks(f.ldv, G);
  // eight 16-byte loads in flight per lane and 512 workgroups: at c4 2167 it/s against 2068 with four loads, 1821 with
  // eight loads on 256 workgroups and 1336 with four on 256 (profiles/screen4_ab.txt); every wave owns one list segment and
  // one of the BCX_MAX_PARTIALS partials
  const int ur = CH == 1 ? 8 : 4;
  const int rpb = BCX_SCREEN_WAVES * (64 / G) * ur;
  const int64_t want = (n + rpb - 1) / rpb;
  int cap = 512;
  if (cap > BCX_MAX_PARTIALS / BCX_SCREEN_WAVES) cap = BCX_MAX_PARTIALS / BCX_SCREEN_WAVES;
  const int grid = (int)(want < 1 ? 1 : (want > cap ? cap : want));
  // (thresh4_kernel goes first in the stream; it is launched here because it books the previous iteration's counts)
  t.counts = (const int*)s->s4_counts; t.n_seg = s->s4_n_seg; t.seg_cap = s->s4_seg_cap;
  f.seg_cap = s->s4_seg_cap;
  hipLaunchKernelGGL(thresh4_kernel, dim3(1), dim3(BCX_THRESH_THREADS), 0, s->stream, t);
  BCX_HIP(hipGetLastError());
  s->s4_n_seg = grid * BCX_SCREEN_WAVES;
  if ((rc = launch_front4(s, f, G, CH, ur, grid))) return rc;

  const int n_in = grid * BCX_SCREEN_WAVES;
  Second8Args c;
  c.Aq = (const uint4*)s->Aq; c.sb = (const float2*)s->scr_sb; c.q = (const float*)s->qst; c.st = s->st;
  c.list = (const int*)s->s4_list; c.counts = (const int*)s->s4_counts;
  c.out = partial_view(s->scr_partials, n_in);
  c.ldv = ldv8; c.d = d; c.seg_cap = s->s4_seg_cap; c.kacc = kacc; c.err_coef = sa.err_coef;
  if ((rc = launch_second8(s, c, G8, CH8, grid))) return rc;
  BCX_HIP(hipGetLastError());
  s->scr_n_in = n_in;
  return bcx_launch_refine(s, n_in);
}
