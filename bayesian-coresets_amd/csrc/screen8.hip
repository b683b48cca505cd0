// screen8.hip -- the 8-bit screening tier of the correlation scan.
//
// The interval scan of scan.hip does not decide the arg-max: it only has to give every row an interval that CONTAINS its
// exact score, and resolve_core re-scores in fp64 the rows whose upper bound reaches the largest lower bound.  The interval
// has to be valid, not narrow -- so the array that is streamed every greedy iteration can be much coarser than the stored
// rows.  This file keeps a third, coarsest copy of the rows ("shadow"), one byte per element, and three kernels:
//
//   quantise_kernel : stored row a (fp32 / fp16, already normalised) -> codes u_j in [1, 255], one fp32 scale per row and
//                     one fp32 UPPER bound of || a - deq(u) ||_2 per row, deq(u)_j = (u_j - 128) * scale
//                       m     = max_j |a_j|                       (exact in fp32)
//                       scale = fp32( double(m) / 127 ), at least FLT_MIN
//                       u_j   = 128 + clamp( rint( double(a_j) / double(scale) ), -127, 127 )     (ties to even)
//                       bound = fp32 round-up of sqrt( sum_j (a_j - (u_j-128)*scale)^2 ) * (1 + 2^-20), summed in fp64
//                     (tests/test_screen8_bound.py restates this in NumPy; bytes between d and the row stride hold 128)
//   screen_kernel   : scan_kernel's structure (16-byte non-temporal loads, G lanes per row, query in registers, transposed
//                     butterflies, top-2 tracks) over the codes.  A lane's accumulator starts at -128 * (sum of its own query
//                     values), so  acc = sum_j (u_j - 128) q_j  and  score8 = scale * acc.
//   refine_kernel   : one workgroup.  Rows whose 8-bit upper bound reaches the largest 8-bit lower bound ("survivors") are
//                     re-scored from the STORED rows with an interval no wider than the storage-precision scan's, and leave
//                     as one partial each in the format resolve_core reads.  resolve_core, the fp64 re-score and the state
//                     update are untouched: they see fewer, tighter partials than scan_kernel would have given them.
//                     For the 4-bit front tier (screen4.hip) it also leaves the next front pass's 64 sentinel rows, picked
//                     from the partials it holds anyway, and books that tier's counters from the list counts.
//
// The enclosure.  Exact score s* = a* . q* (a*: the exact normalised row, q*: the fp64 query); a~, q~: their stored / fp32
// roundings; deq: the dequantised row.  With qs = |q| (DevState::qscale):
//   |score8 - s*| <= |score8 - deq.q~|  +  |deq.q~ - a~.q~|  +  |a~.q~ - s*|
//   (3) storage rounding of row and query: inside err_coef * qs of bcx_scan_plan (which also covers a summation we do not do)
//   (2) Cauchy-Schwarz: || deq - a~ ||_2 |q~| <= bound[n] * qs
//   (1) fp32 accumulation over integers.  Per lane: nq = 16 CH fused multiply-adds on top of the start value, whose own
//       sum of nq query values carries gamma_nq * 128 * sum|q|; terms |u_j q_j| <= 255 |q_j| and 128 |q_j|:
//         lane error   <= gamma_{nq+1} * (255 + 128 + 128) * sum_lane |q~_j|
//         butterfly    <= lg(G) * u * 127 * sum |q~_j|               (partial sums are bounded by 127 sum|q~_j|)
//       with sum |q~_j| <= sqrt(d) * qs and u = 2^-24, times the row's scale:
//         kacc = 1.3 * u * (511 * (16 CH + 1) + 127 lg G) * sqrt(d)      (30 % head room for the second-order terms)
//       The final multiply by the scale rounds by u |score8|: the 2e-7 |s| term every fp32 interval here already carries.
//   e[n] = ((bound[n] + scale[n] * kacc) * (1 + 2e-6) + err_coef) * qs     (the factor covers this expression's own rounding
//                                                                            and the fp32 rounding of qs)
// For GIGA both queries have unit norm and giga_interval takes the same e for s0 and s1, as in scan_kernel.
//
// Capture.  Every WAVE (not workgroup) reports its two largest upper bounds, a bound on its other rows and its largest lower
// bound: 4 x the bins of scan_kernel for the same launch width.  A third survivor inside one wave, or more than
// BCX_SCREEN_MAX_SURV survivors, is an overflow: the refine kernel hands resolve_core a partial that makes it report
// BCX_REC_OVERFLOW, the state machine halts as for a candidate-window overflow, and bcx_build_poll redoes that iteration with
// the storage-precision scan (api.hip).  tools/screen8_model.py emulates this capture; DESIGN.md 4.1 has its numbers.
//
// The scoring and interval code (Q16, dot16, load_q16, screen_interval) lives in screen_core.h: the 4-bit front pass
// (screen4.hip) scores its listed rows with the same text, inside its own launch, and hands its partials to refine_kernel here.
#include <float.h>
#include "screen_core.h"

#define BCX_REFINE_THREADS 1024

struct ScreenArgs {
  const uint4* Aq;     // n x ldv pieces of 16 codes
  const float2* sb;    // per row: (scale, bound)
  const float* q;      // query 0 at q, query 1 at q + ldq (fp32)
  const DevState* st;
  PartialView out;     // one partial per wave
  int64_t n;
  int ldv;             // pieces per row
  int ldq;
  int d;
  float kacc;          // accumulation term per unit of scale and qscale (see the head of this file)
  float err_coef;      // the storage tier's own term
};

template <bool DUAL, int G, int CH, int UR>
__global__ __launch_bounds__(BCX_SCAN_THREADS) void screen_kernel(ScreenArgs a) {
  if (!a.st->active) return;
  constexpr int RPW = 64 / G;                       // rows per wave per step
  constexpr int WAVES = BCX_SCREEN_WAVES;
  constexpr int RPB = WAVES * RPW * UR;             // rows per workgroup per trip
  constexpr bool PACK4 = G >= 4 && (UR % 4 == 0);
  constexpr int GSZ = PACK4 ? G / 4 : G;            // lanes that end up tracking the same row
  constexpr int NT = PACK4 ? UR / 4 : UR;           // rows a lane tracks per trip
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int sub = lane % G, rsub = lane / G;
  int myu = 0, myrs = 0;
  if constexpr (PACK4) pack_map<G>(lane, myu, myrs);

  Q16 q0[CH], q1[CH];
  int voff[CH];
  float qs0 = 0.0f, qs1 = 0.0f;
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    const int v = c * G + sub;
    const bool ok = v < a.ldv;
    voff[c] = ok ? v : 0;     // clamp: the load stays inside the row, the zero query kills the product
    q0[c] = load_q16(a.q, v, a.d, ok, qs0);
    if (DUAL) q1[c] = load_q16(a.q + a.ldq, v, a.d, ok, qs1);
  }
  const float off0 = -128.0f * qs0, off1 = -128.0f * qs1;   // (x 128: exact)
  const float qscale = (float)a.st->qscale;

  Track<float> tr;
  tr.U1 = tr.U2 = tr.U3 = tr.L = -INFINITY;
  tr.i1 = tr.i2 = 0x7fffffff;

  const uint4* base = a.Aq;
  const int64_t n = a.n;
  auto row_of = [&](int64_t r0, int u) { return r0 + (int64_t)(u * WAVES + wave) * RPW + rsub; };
  auto tracked = [&](int64_t r0, int t) {           // the row whose total this lane holds after the reduction
    if constexpr (PACK4) return r0 + (int64_t)((t * 4 + myu) * WAVES + wave) * RPW + myrs;
    else return row_of(r0, t);
  };
  const int64_t stride = (int64_t)gridDim.x * RPB;
  for (int64_t r0 = (int64_t)blockIdx.x * RPB; r0 < n; r0 += stride) {
    uint4 x[UR][CH];
    float2 sbv[NT];
#pragma unroll
    for (int u = 0; u < UR; ++u) {
      const int64_t rw = row_of(r0, u);
      const int64_t rc = rw < n ? rw : n - 1;
      const uint4* p = base + rc * a.ldv;
#pragma unroll
      for (int c = 0; c < CH; ++c) x[u][c] = stream_load(p + voff[c]);
    }
#pragma unroll
    for (int t = 0; t < NT; ++t) { const int64_t rw = tracked(r0, t); sbv[t] = a.sb[rw < n ? rw : n - 1]; }
    __builtin_amdgcn_sched_barrier(0);   // all loads of the trip in flight before the first use (see scan_kernel)
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      float s0, s1 = 0.0f;
      if constexpr (PACK4) {
        float a0[4], a1[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          float t0 = off0, t1 = off1;
#pragma unroll
          for (int c = 0; c < CH; ++c) {
            t0 = dot16(x[t * 4 + u][c], q0[c], t0);
            if (DUAL) t1 = dot16(x[t * 4 + u][c], q1[c], t1);
          }
          a0[u] = t0; a1[u] = t1;
        }
        s0 = reduce4_pack<G, float>(a0[0], a0[1], a0[2], a0[3]);
        if (DUAL) s1 = reduce4_pack<G, float>(a1[0], a1[1], a1[2], a1[3]);
      } else {
        float t0 = off0, t1 = off1;
#pragma unroll
        for (int c = 0; c < CH; ++c) {
          t0 = dot16(x[t][c], q0[c], t0);
          if (DUAL) t1 = dot16(x[t][c], q1[c], t1);
        }
        s0 = group_allsum<float, G>(t0);
        if (DUAL) s1 = group_allsum<float, G>(t1);
      }
      const int64_t myrow = tracked(r0, t);
      const float scale = sbv[t].x, bound = sbv[t].y;
      s0 *= scale; s1 *= scale;
      float U, L;
      if (DUAL) giga_interval(s0, s1, (fmaf(scale, a.kacc, bound) * 1.000002f + a.err_coef) * qscale, U, L);
      else screen_interval(s0, scale, bound, a.kacc, a.err_coef, qscale, U, L);
      if (!(myrow < n)) { U = -INFINITY; L = -INFINITY; }
      track_update<float>(tr, U, L, (int)myrow);
    }
  }
  // combine the row groups of a wave; every wave reports on its own
#pragma unroll
  for (int off = GSZ; off < 64; off <<= 1) tr = merge<float>(tr, shfl_track<float>(tr, off));
  if (lane == 0) {
    const int b = blockIdx.x * WAVES + wave;
    a.out.U1[b] = (double)tr.U1; a.out.U2[b] = (double)tr.U2; a.out.U3[b] = (double)tr.U3; a.out.L[b] = (double)tr.L;
    a.out.i1[b] = tr.i1; a.out.i2[b] = tr.i2;
  }
}

// ---- survivors -> storage-precision partials ------------------------------------------------------------------------
struct RefineArgs {
  PartialView in;       // the screen kernel's partials
  int n_in;
  PartialView out;      // BCX_SCREEN_MAX_SURV partials for resolve_core
  DevState* st;
  unsigned long long* stat;   // ScreenStat words (bcx_internal.h)
  const void* An;
  const float* q;
  int store_f16, ld, ldq, d, dual;
  double coef_mid;      // |fp64-accumulated stored score - exact score| <= coef_mid * qscale
  // the 4-bit front tier (screen4.hip); sent is null when the solver has no 4-bit shadow
  int* sent;            // out: BCX_S4_SENTINELS row indices for the next front pass, -1: none
  const int* counts;    // the list counts the front pass of THIS iteration wrote, one per partial; null: a plain 8-bit iteration
  int seg_cap;          // entries of a list segment in use
  int64_t n;
};

#define BCX_REFINE_PF 8   // elements per lane of a wave's first survivor row that are loaded ahead of the sentinel selection

__global__ __launch_bounds__(BCX_REFINE_THREADS) void refine_kernel(RefineArgs a) {
  if (!a.st->active) return;
  __shared__ double scratch[BCX_SCRATCH];
  __shared__ int surv[BCX_SCREEN_MAX_SURV];
  __shared__ int nsurv, overflow, listed, full;
  constexpr int PP = BCX_MAX_PARTIALS / BCX_REFINE_THREADS;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nwaves = BCX_REFINE_THREADS / 64;
  double u1[PP], u2[PP], u3[PP], lo[PP];
  int r1[PP], r2[PP], cn[PP];
#pragma unroll
  for (int t = 0; t < PP; ++t) {
    const int p = tid + t * BCX_REFINE_THREADS;
    const bool ok = p < a.n_in;
    u1[t] = ok ? a.in.U1[p] : -INFINITY; u2[t] = ok ? a.in.U2[p] : -INFINITY;
    u3[t] = ok ? a.in.U3[p] : -INFINITY; lo[t] = ok ? a.in.L[p] : -INFINITY;
    r1[t] = ok ? a.in.i1[p] : 0; r2[t] = ok ? a.in.i2[p] : 0;
    cn[t] = (ok && a.counts) ? a.counts[p] : 0;
  }
  if (tid == 0) { nsurv = 0; overflow = 0; listed = 0; full = 0; }
  double lmax = -INFINITY;
#pragma unroll
  for (int t = 0; t < PP; ++t) lmax = fmax(lmax, lo[t]);
  const double Lstar = block_allmax(lmax, scratch);    // (its barriers also publish nsurv / overflow)
#pragma unroll
  for (int t = 0; t < PP; ++t) {
    if (u1[t] > -INFINITY && u1[t] >= Lstar) { const int s = atomicAdd(&nsurv, 1); if (s < BCX_SCREEN_MAX_SURV) surv[s] = r1[t]; }
    if (u2[t] > -INFINITY && u2[t] >= Lstar) { const int s = atomicAdd(&nsurv, 1); if (s < BCX_SCREEN_MAX_SURV) surv[s] = r2[t]; }
    if (u3[t] > -INFINITY && u3[t] >= Lstar) overflow = 1;
  }
  if (a.counts) {   // (kernel-uniform) rows listed and full segments of this iteration's front pass: exact in a double
    double li = 0.0, fu = 0.0;
#pragma unroll
    for (int t = 0; t < PP; ++t) { li += (double)(cn[t] > a.seg_cap ? a.seg_cap : cn[t]); fu += cn[t] > a.seg_cap ? 1.0 : 0.0; }
    li = wave_allsum(li); fu = wave_allsum(fu);
    if (lane == 0) { atomicAdd(&listed, (int)li); atomicAdd(&full, (int)fu); }
  }
  __syncthreads();
  const int ns = nsurv;
  const bool ovf = overflow || ns > BCX_SCREEN_MAX_SURV;
  // unused output partials: nothing there
  for (int p = tid; p < BCX_SCREEN_MAX_SURV; p += BCX_REFINE_THREADS) {
    if (ovf || p >= ns) {
      // overflow: partial 0 claims unseen rows above its lower bound, which resolve_core reports as BCX_REC_OVERFLOW
      const bool mark = ovf && p == 0;
      a.out.U1[p] = -INFINITY; a.out.U2[p] = -INFINITY; a.out.U3[p] = mark ? INFINITY : -INFINITY; a.out.L[p] = mark ? 0.0 : -INFINITY;
      a.out.i1[p] = 0x7fffffff; a.out.i2[p] = 0x7fffffff;
    }
  }
  if (tid == 0) {   // (fire-and-forget atomics: a read-modify-write would stall wave 0 for a memory round trip)
    a.stat[SCR_ARMED] = 1ull;
    atomicAdd(&a.stat[SCR_ITERS], 1ull);
    if (ovf) atomicAdd(&a.stat[SCR_OVERFLOWS], 1ull); else atomicAdd(&a.stat[SCR_SURVIVORS], (unsigned long long)ns);
    a.stat[SCR4_LAST] = a.counts ? 1ull : 0ull;
    if (a.counts) {
      atomicAdd(&a.stat[SCR4_ITERS], 1ull);
      atomicAdd(&a.stat[SCR4_LISTED], (unsigned long long)listed);
      atomicAdd(&a.stat[SCR4_OVERFLOWS], (unsigned long long)full);
    }
  }
  auto stored = [&](int64_t i, int j) -> double {
    return a.store_f16 ? (double)__half2float(((const __half*)a.An)[i * (int64_t)a.ld + j])
                       : (double)((const float*)a.An)[i * (int64_t)a.ld + j];
  };
  // the head of this wave's first survivor row (and the query beside it) is requested before the sentinel selection, which
  // needs no memory: unconditional loads at clamped addresses, so that all of them are in flight together.  (Without a 4-bit
  // tier there is no selection to hide, and the rows are read by the loop below as before.)
  double pv[BCX_REFINE_PF];
  float pq0[BCX_REFINE_PF];
  const bool ahead = a.sent && !a.dual && !ovf && wave < ns;   // (kernel-uniform but for the wave; the path sums one query only)
#pragma unroll
  for (int k = 0; k < BCX_REFINE_PF; ++k) { pv[k] = 0.0; pq0[k] = 0.0f; }
  if (ahead) {
    const int64_t row0 = surv[wave];
#pragma unroll
    for (int k = 0; k < BCX_REFINE_PF; ++k) {
      const int j = lane + 64 * k, jc = j < a.d ? j : 0;
      pv[k] = stored(row0, jc); pq0[k] = a.q[jc];
    }
  }
  __builtin_amdgcn_sched_barrier(0);
  // The next front pass's sentinels (screen4.hip): this wave's SPW largest upper bounds among the 2 PP x 64 candidates it holds
  // -- 16 x 4 rows, the 4 largest of all among them.  Written on every path that leaves tier partials, overflow included.
  if (a.sent) {
    constexpr int SPW = BCX_S4_SENTINELS / (BCX_REFINE_THREADS / 64);
    double cu[2 * PP];
    int ci[2 * PP];
#pragma unroll
    for (int t = 0; t < 2 * PP; ++t) {
      const double u = (t & 1) ? u2[t >> 1] : u1[t >> 1];
      const int i = (t & 1) ? r2[t >> 1] : r1[t >> 1];
      const bool use = u > -INFINITY && u < INFINITY && i >= 0 && (int64_t)i < a.n;   // (false for NaN)
      cu[t] = use ? u : -INFINITY; ci[t] = use ? i : -1;
    }
#pragma unroll
    for (int r = 0; r < SPW; ++r) {
      double best = -INFINITY;
      int bt = -1, bi = -1;
#pragma unroll
      for (int t = 0; t < 2 * PP; ++t) if (cu[t] > best) { best = cu[t]; bt = t; bi = ci[t]; }
      const double wm = wave_allmax(best);
      const unsigned long long bal = __ballot(bt >= 0 && best == wm);
      const int src = bal ? __ffsll((long long)bal) - 1 : 0;
      const int row = __shfl(bi, src, BCX_WAVE);
      if (lane == 0) a.sent[wave * SPW + r] = bal ? row : -1;   // -1: no candidates left
#pragma unroll
      for (int t = 0; t < 2 * PP; ++t) if (bal && lane == src && t == bt) cu[t] = -INFINITY;
    }
  }
  if (ovf) return;
  const double qs = a.st->qscale;
  const double e = a.coef_mid * qs;
  for (int c = wave; c < ns; c += nwaves) {
    const int64_t i = surv[c];
    double s0 = 0.0, s1 = 0.0;
    int j = lane;
    if (ahead && c == wave) {   // (same order of the sum as the loop below)
#pragma unroll
      for (int k = 0; k < BCX_REFINE_PF; ++k, j += 64) {
        const double t0 = fma(pv[k], (double)pq0[k], s0);
        s0 = j < a.d ? t0 : s0;
      }
    }
    for (; j < a.d; j += 64) {
      const double v = stored(i, j);
      s0 = fma(v, (double)a.q[j], s0);
      if (a.dual) s1 = fma(v, (double)a.q[a.ldq + j], s1);
    }
    s0 = wave_allsum(s0);
    if (a.dual) s1 = wave_allsum(s1);
    if (lane == 0) {
      double U, L;
      if (a.dual) {
        // (the conversions to fp32 round by u |s| <= u: inside e, whose 30 % head room is 0.9 u at least)
        float Uf, Lf;
        giga_interval((float)s0, (float)s1, (float)(e * 1.000001) , Uf, Lf);
        U = Uf; L = Lf;
      } else { U = s0 + e; L = s0 - e; }
      a.out.U1[c] = U; a.out.L[c] = L; a.out.i1[c] = (int)i;
      a.out.U2[c] = -INFINITY; a.out.U3[c] = -INFINITY; a.out.i2[c] = 0x7fffffff;
    }
  }
}

// a halted tier iteration is redone with the storage-precision scan: not an exact fallback (n_exact stays)
__global__ __launch_bounds__(64) void resume_store_kernel(DevState* st, unsigned long long* stat) {
  if (threadIdx.x == 0 && st->halt == HALT_NEED_EXACT && stat[SCR_ARMED]) {
    st->active = 1; st->halt = HALT_NONE; st->exact_mode = 0;
    stat[SCR_ARMED] = 0ull; stat[SCR_REDOS] += 1ull;
  }
}

// ---- quantiser ------------------------------------------------------------------------------------------------------
// one wave per row; a lane owns words of 4 consecutive elements
template <bool F16>
__global__ __launch_bounds__(256) void quantise_kernel(const void* An, int ld, int d, int ld8, int64_t n, unsigned* Aq, float2* sb) {
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
  float sc = (float)((double)m / 127.0);
  if (!(sc >= FLT_MIN)) sc = FLT_MIN;
  const double dsc = (double)sc;
  double r2 = 0.0;
  const int nw = ld8 / 4;
  for (int w = lane; w < nw; w += 64) {
    unsigned word = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int j = 4 * w + k;
      int code = 0;
      if (j < d) {
        const double v = (double)elem(j);
        double c = rint(v / dsc);
        c = c > 127.0 ? 127.0 : (c < -127.0 ? -127.0 : c);
        if (c != c) c = 0.0;
        code = (int)c;
        const double r = v - c * dsc;
        r2 = fma(r, r, r2);
      }
      word |= (unsigned)(code + 128) << (8 * k);
    }
    Aq[row * (int64_t)nw + w] = word;
  }
  r2 = wave_allsum(r2);
  if (lane == 0) {
    const double b = sqrt(r2) * (1.0 + 9.5367431640625e-07);
    float bf = (float)b;
    if ((double)bf < b) bf = nextafterf(bf, INFINITY);
    if (!(bf == bf)) bf = INFINITY;      // NaN in the row: its interval is everything, the fp64 stage decides
    sb[row] = make_float2(sc, bf);
  }
}

// ---- host side --------------------------------------------------------------------------------------------------------
static bool screen_applicable(const bcx_solver* s) {
  // fp32 / fp16 storage; rows of at most 64 x 4 pieces (d <= 4096): beyond, the query no longer fits the registers
  return s->cfg.store_dtype != BCX_F64 && s->cfg.d <= 64 * 4 * 16 && s->cfg.n_local > 0;
}

bool bcx_screen_on(const bcx_solver* s) { return s->scr_enabled && !s->scr_dropped && screen_applicable(s); }

// Build (or rebuild after a reload) the shadow of the stored rows.  Lazily, before the first enqueued iteration after
// bcx_finalize: solvers that never run bcx_build_enqueue (the select step of SparseVI) never pay for it.
int bcx_screen_build(bcx_solver* s) {
  if (s->scr_valid || !bcx_screen_on(s)) return BCX_OK;
  const int d = s->cfg.d;
  const int64_t n = s->cfg.n_local;
  s->ld8 = (d + 15) / 16 * 16;
  if (s->scr_sb.count() < (size_t)n || !s->Aq) {
    s->Aq.reset(); s->scr_sb.reset();      // both go before either is asked for again
    if (s->Aq.alloc((size_t)n * s->ld8, false) || s->scr_sb.alloc((size_t)n, false) ||
        (!s->scr_partials && s->scr_partials.alloc((size_t)BCX_MAX_PARTIALS * BCX_PARTIAL_BYTES, false)) ||
        (!s->scr_stat && s->scr_stat.alloc(SCR_WORDS, true))) {
      // no room for the shadow: the solver runs on the storage-precision scan, and says so in bcx_screen_stats
      (void)hipGetLastError();
      s->Aq.reset(); s->scr_sb.reset();
      s->scr_dropped = 2;
      return BCX_OK;
    }
  }
  hipEvent_t e0, e1;
  BCX_HIP(hipEventCreate(&e0));
  BCX_HIP(hipEventCreate(&e1));
  BCX_HIP(hipEventRecord(e0, s->stream));
  const unsigned grid = (unsigned)((n + 3) / 4);
  if (s->cfg.store_dtype == BCX_F16)
    hipLaunchKernelGGL((quantise_kernel<true>), dim3(grid), dim3(256), 0, s->stream, s->An, s->ld, d, s->ld8, n, (unsigned*)s->Aq.get(), s->scr_sb.get());
  else
    hipLaunchKernelGGL((quantise_kernel<false>), dim3(grid), dim3(256), 0, s->stream, s->An, s->ld, d, s->ld8, n, (unsigned*)s->Aq.get(), s->scr_sb.get());
  BCX_HIP(hipGetLastError());
  BCX_HIP(hipEventRecord(e1, s->stream));
  BCX_HIP(hipEventSynchronize(e1));
  float ms = 0.f;
  BCX_HIP(hipEventElapsedTime(&ms, e0, e1));
  (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
  s->scr_build_ms = ms;
  s->scr_valid = true;
  return BCX_OK;
}

template <bool DUAL> static int launch_screen_t(bcx_solver* s, const ScreenArgs& a, int G, int CH, int UR, int grid) {
  dim3 g(grid), b(BCX_SCAN_THREADS);
#define L(GG, CC, UU)                                                                            \
  if (G == GG && CH == CC && UR == UU) {                                                         \
    hipLaunchKernelGGL((screen_kernel<DUAL, GG, CC, UU>), g, b, 0, s->stream, a);                \
    return BCX_OK;                                                                               \
  }
  L(1, 1, 4) L(2, 1, 4) L(4, 1, 4) L(8, 1, 4) L(16, 1, 4) L(32, 1, 4) L(64, 1, 4) L(64, 2, 4) L(64, 4, 4)
  L(4, 1, 8) L(8, 1, 8) L(16, 1, 8) L(32, 1, 8) L(64, 1, 8)
#undef L
  s->err = "screen: unsupported row length";
  return BCX_ERR_ARG;
}

// One tier iteration's front: the 8-bit scan and the refine kernel.  Afterwards s->partials / s->n_partials describe
// BCX_SCREEN_MAX_SURV storage-precision partials, exactly what the tail kernels read after bcx_launch_scan.
int bcx_launch_screen(bcx_solver* s) {
  const int d = s->cfg.d;
  ScreenArgs a;
  a.Aq = (const uint4*)s->Aq.get();
  a.sb = s->scr_sb;
  a.q = (const float*)s->qst.get();
  a.ldq = s->ld;
  a.st = s->st;
  a.n = s->cfg.n_local;
  a.ldv = s->ld8 / 16;
  a.d = d;
  const int G = screen_group(a.ldv);
  const int CH = screen_chunks(a.ldv, G);
  a.kacc = screen_kacc(G, CH, d);
  // the storage tier's own term, as bcx_scan_plan states it for the stored rows
  ScanArgs sa;
  ScanPlan sp;
  int rc = bcx_scan_plan(s, 0, &sa, &sp);
  if (rc != BCX_OK) return rc;
  a.err_coef = sa.err_coef;
  int ur = 4;
  if (const char* e = bcx_dev_env("BCX_SCREEN_UR")) { if (atoi(e) == 8 && CH == 1 && G >= 4) ur = 8; }
  // launch width: scan_grid_for's rule (about 32 KiB of loads in flight per CU), at most 512 workgroups: every wave owns
  // one of the BCX_MAX_PARTIALS partials
  const int rpb = BCX_SCREEN_WAVES * (64 / G) * ur;
  int64_t want = (a.n + rpb - 1) / rpb;
  int cap = (CH * ur >= 8) ? 256 : 512;
  if (const char* e = bcx_dev_env("BCX_SCREEN_GRID")) { const long v = atol(e); if (v > 0) cap = (int)v; }
  if (cap > BCX_MAX_PARTIALS / BCX_SCREEN_WAVES) cap = BCX_MAX_PARTIALS / BCX_SCREEN_WAVES;
  const int grid = (int)(want < 1 ? 1 : (want > cap ? cap : want));
  const int n_in = grid * BCX_SCREEN_WAVES;
  a.out = partial_view(s->scr_partials, n_in);
  const bool dual = s->cfg.alg == BCX_ALG_GIGA;
  rc = dual ? launch_screen_t<true>(s, a, G, CH, ur, grid) : launch_screen_t<false>(s, a, G, CH, ur, grid);
  if (rc != BCX_OK) return rc;
  s->scr_n_in = n_in;
  return bcx_launch_refine(s, n_in, false);
}

// The refine kernel over the n_in per-wave partials in s->scr_partials (written by screen_kernel, or by the second stage of
// the 4-bit tier in the same format; four: the latter, whose list counts the kernel then books).
int bcx_launch_refine(bcx_solver* s, int n_in, bool four) {
  const int d = s->cfg.d;
  const bool f16 = s->cfg.store_dtype == BCX_F16;
  const double u = 5.9604644775390625e-08;
  RefineArgs r;
  r.in = partial_view(s->scr_partials, n_in); r.n_in = n_in;
  r.out = partial_view(s->partials, BCX_SCREEN_MAX_SURV);
  r.st = s->st; r.stat = s->scr_stat;
  r.An = s->An; r.q = (const float*)s->qst.get();
  r.store_f16 = f16; r.ld = s->ld; r.ldq = s->ld; r.d = d; r.dual = s->cfg.alg == BCX_ALG_GIGA;
  r.sent = bcx_screen4_on(s) ? s->s4_sent.get() : nullptr;   // (dropped to the 8-bit tier: nobody reads sentinels until reset)
  r.counts = four ? s->s4_counts.get() : nullptr; r.seg_cap = s->s4_seg_cap; r.n = s->cfg.n_local;
  // stored row and fp32 query multiplied and summed in fp64: what is left is their own rounding (2 u, fp16: its storage term)
  // and d 2^-53; 30 % head room as in bcx_scan_plan
  r.coef_mid = 1.3 * u * 3.0;
  if (f16) r.coef_mid += 1.02 * (4.8828125e-4 + 2.9802322387695312e-08 * sqrt((double)d));
  hipLaunchKernelGGL(refine_kernel, dim3(1), dim3(BCX_REFINE_THREADS), 0, s->stream, r);
  BCX_HIP(hipGetLastError());
  s->n_partials = BCX_SCREEN_MAX_SURV;
  return BCX_OK;
}

int bcx_launch_resume_store(bcx_solver* s) {
  hipLaunchKernelGGL(resume_store_kernel, dim3(1), dim3(64), 0, s->stream, s->st, s->scr_stat);
  BCX_HIP(hipGetLastError());
  return BCX_OK;
}

