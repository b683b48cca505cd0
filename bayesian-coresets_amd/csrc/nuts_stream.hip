// nuts_stream.hip -- the No-U-Turn transition of csrc/nuts.hip for rows that do not fit one workgroup's LDS
// (coresets past it, the resident full data set): the same transition, noise layout, dual averaging, outputs and status word,
// the N rows STREAMED from device memory by G co-resident workgroups in ONE persistent launch for all chains and transitions
// (the form of csrc/laplace_stream.hip: the bounded grid barriers of nnls_common.h, partial records added in workgroup order).
//
// A ROUND evaluates one leaf for every chain that is still running:
//  * pass (all workgroups): a workgroup owns a contiguous range of 128-row tiles and evaluates it against the theta of the
//    ACTIVE chains, 8 columns at a time, with the two phases of lj_partial_kernel (csrc/hmc.hip): row x 4 columns -> lap_point,
//    w g to LDS; column x coordinate -> the outer-product sum.  One record [sum w g x (D) | sum w log p] per workgroup and
//    active chain goes to half round & 1 of part[2][G][C][D + 1].  Every workgroup forms the same active list from the
//    per-chain flags; a list that is no multiple of 8 is padded with theta = 0 columns whose sums are not written.  BARRIER.
//  * consume (the chain's owner, workgroup c mod G; a workgroup that owns several gives them to its four waves in turn, each
//    wave moving its chains on by itself, a lane per coordinate, with no workgroup barrier inside): adds the G records of the chain in
//    workgroup order (sc1 loads, no floating-point atomics), applies the prior, takes g_xi = W g_theta and runs the NUTS
//    state machine ONE LEAF forward from the chain's record in the scratch: finishes the leaf (second half kick, energy,
//    accept statistic, divergence, leaf selection, checkpoint or span tests); where the leaf closes a doubling, the tree-level
//    selection, the endpoint replacement and the tree's own turn test; where that ends the transition, the outputs, the dual
//    averaging and the set-up of transition t + 1 from its noise row.  Then the first half kick and drift of the next leaf,
//    whose theta goes to Theta[c] -- or, after transition T, the chain's flag is cleared.  BARRIER.
//  * every workgroup reads the C flags and leaves when none is set.
// Round 0 evaluates the start state xi = 0 (theta = mu) of every chain.  The round loop is bounded by 1 + T (2^J - 1); a chain
// that ends a transition early starts its next one in the next round, and the launch ends with its slowest chain.
//
// Why no buffer is rewritten before its last reader has passed a barrier.  Round r has barriers 2 r + 1 (after the pass) and
// 2 r + 2 (after the consume); every workgroup passes every barrier exactly once and in order, so none is ever more than one
// barrier ahead of another (the invariant grid_barrier rests on).
//  * part, half r & 1: written in the pass of round r, read by the owners between barriers 2 r + 1 and 2 r + 2.  Its next
//    writer is the pass of round r + 2, behind barrier 2 r + 4, which no workgroup passes before every owner has arrived at
//    2 r + 2, its reads done.
//  * Theta[c] and the flag of chain c: written by the owner between barriers 2 r + 1 and 2 r + 2; read by every workgroup
//    behind 2 r + 2 (the flags for the active list, Theta in the pass of round r + 1) and before it arrives at 2 r + 3.  The
//    owner writes them again only behind 2 r + 3, at which every reader has arrived.
//  * a chain's record: read and written by its owner alone, always the same workgroup; a release / acquire pair of the barrier
//    lies between a write and the next read.
//  * the active list (LDS) is rebuilt behind barrier 2 r + 2 from flags nobody writes before 2 r + 3.
#include <algorithm>
#include <string>
#include "bcx_internal.h"
#include "nnls_common.h"
#include "hmc_core.h"
#include "nuts_core.h"
#include "launch_host.h"

#define NS_THREADS 256
#define NS_WAVES (NS_THREADS / 64)
#define NS_ROWS 128             // rows of a tile
#define NS_CT 8                 // theta columns of a pass over the workgroup's tiles
#define NS_MAX_WGS 256          // the owner of a chain adds one record per workgroup
#define NS_CMAX 256             // chains (HMC_STREAM_CMAX of csrc/hmc.hip)
#define NS_SYNC_BYTES 128       // the arrival counter, alone in the first 128 bytes of the scratch (zeroed before every launch)
#define NS_TREE_FIXED (10 * 32) // doubles of NutsTree ahead of its checkpoints

// a chain's record in the scratch: HmcChain | NutsTree without the checkpoints | J checkpoints of xi | J of the momentum |
// NS_SC scalars | NI_COUNT integers
enum { NS_LOGP = 0, NS_H0, NS_LOGW, NS_LOGS, NS_ASUM, NS_DSEL, NS_BASE, NS_HBAR, NS_LEBAR, NS_ACC, NS_LOGPS, NS_HS, NS_SC = 16 };
enum { NI_PH = 0, NI_T, NI_J, NI_I, NI_NLEAF, NI_DEPTH, NI_DIV, NI_COUNT = 8 };      // NI_PH: 0 the start state is being evaluated, 1 a leaf
#define NS_CHAIN_DOUBLES ((int)(sizeof(HmcChain) / sizeof(double)))
static __host__ __device__ inline int ns_record_doubles(int J) { return NS_CHAIN_DOUBLES + NS_TREE_FIXED + 2 * J * 32 + NS_SC + NI_COUNT / 2; }

struct NsArgs {
  HmcPar par;           // (noise: C x T rows of stride noise_ld; L unused; diag: C x T x 8)
  const double* w;      // N weights or NULL (ones)
  const double* Z;      // N x ldz
  int* flags;           // NS_CMAX: chain c still has a leaf to evaluate
  double* Theta;        // C x 32: the point the next pass evaluates for chain c
  double* recs;         // C x rec: the chains' records
  double* part;         // 2 x G x C x (D + 1)
  int64_t N, ldz, noise_ld;
  int family, J, rec;
};

// the lanes of ONE wave are in step, but the compiler must keep their LDS accesses on either side of this in order
static __device__ __forceinline__ void ns_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// a record between the scratch and a wave's LDS copy (all 64 lanes of the wave)
static __device__ __forceinline__ void ns_record_io(double* rec, HmcChain& Sc, NutsTree& Tr, int J, bool store) {
  const int lane = threadIdx.x & 63;
  double* chain = (double*)&Sc;
  double* tree = (double*)&Tr;
  for (int e = lane; e < NS_CHAIN_DOUBLES; e += 64) { if (store) rec[e] = chain[e]; else chain[e] = rec[e]; }
  double* rt = rec + NS_CHAIN_DOUBLES;
  for (int e = lane; e < NS_TREE_FIXED; e += 64) { if (store) rt[e] = tree[e]; else tree[e] = rt[e]; }
  double* rx = rt + NS_TREE_FIXED;
  double* rp = rx + J * 32;
  for (int e = lane; e < J * 32; e += 64) {
    if (store) { rx[e] = Tr.ckx[e >> 5][e & 31]; rp[e] = Tr.ckp[e >> 5][e & 31]; }
    else { Tr.ckx[e >> 5][e & 31] = rx[e]; Tr.ckp[e >> 5][e & 31] = rp[e]; }
  }
}

__global__ __launch_bounds__(NS_THREADS) void nuts_stream_kernel(NsArgs a, GridSync gs) {
  __shared__ double sX[NS_ROWS * HMC_LDW];
  __shared__ double sG[NS_ROWS * (NS_CT + 1)];         // w_j g_jc of the tile; at the end the threads' value sums (256 x 4)
  __shared__ double sTh[NS_CT * HMC_LDW];
  __shared__ double sw[NS_ROWS], sy[NS_ROWS];
  __shared__ double sW[32 * HMC_LDW], sMu[32];         // the frame
  __shared__ HmcChain sC[NS_WAVES];                     // per wave: the record of the chain it is consuming
  __shared__ NutsTree sT[NS_WAVES];
  __shared__ double s_gth[NS_WAVES][32], s_sc[NS_WAVES][NS_SC], s_val[NS_WAVES];
  __shared__ int s_iv[NS_WAVES][NI_COUNT];
  __shared__ int s_act[NS_CMAX], s_on[NS_CMAX], s_cnt[NS_THREADS / 64];
  __shared__ int s_flag;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wg = blockIdx.x, G = gridDim.x;
  const int D = a.par.D, C = a.par.C, J = a.J, T = a.par.T, nwarm = a.par.nwarm, ld = a.par.ld;
  const int64_t tiles = (a.N + NS_ROWS - 1) / NS_ROWS;
  const int64_t begin = tiles * wg / G * NS_ROWS;
  const int64_t end = tiles * (wg + 1) / G * NS_ROWS < a.N ? tiles * (wg + 1) / G * NS_ROWS : a.N;
  const int r = tid & (NS_ROWS - 1), hq = (tid >> 7) * 4;      // phase A: row r, columns hq .. hq + 3
  const int bc = tid >> 5, bd = tid & 31;                       // phase B: column bc, coordinate bd
  const bool adapt = !(a.par.fixed_eps > 0.0);
  const size_t cstride = (size_t)C * (D + 1);                   // one workgroup's records

  for (int e = tid; e < 32 * 32; e += NS_THREADS) {             // (the frame as hmc_load_frame lays it out)
    const int i = e >> 5, c = e & 31;
    sW[i * HMC_LDW + c] = (i < D && c < D) ? (a.par.W ? a.par.W[(size_t)i * a.par.ldw + c] : (i == c ? 1.0 : 0.0)) : 0.0;
  }
  if (tid < 32) sMu[tid] = (tid < D && a.par.mu) ? a.par.mu[tid] : 0.0;
  __syncthreads();
  HmcChain& Sc = sC[wave];
  NutsTree& Tr = sT[wave];
  double* gth = s_gth[wave];
  // th = mu + W^T xp of the wave's chain (hmc_theta of csrc/hmc_core.h, a lane per coordinate)
  auto theta = [&]() {
    if (lane < D) {
      double v = sMu[lane];
      for (int i = 0; i < D; ++i) v = fma(sW[i * HMC_LDW + lane], Sc.xp[i], v);
      Sc.th[lane] = v;
    }
  };
  // the records of this workgroup's chains at the start state xi = 0; every chain is active in round 0
  for (int c = wg + G * wave; c < C; c += G * NS_WAVES) {
    for (int e = lane; e < NS_CHAIN_DOUBLES; e += 64) ((double*)&Sc)[e] = 0.0;
    for (int e = lane; e < (int)(sizeof(NutsTree) / sizeof(double)); e += 64) ((double*)&Tr)[e] = 0.0;
    ns_wave_sync();
    theta();
    ns_wave_sync();
    double* rec = a.recs + (size_t)c * a.rec;
    ns_record_io(rec, Sc, Tr, J, true);
    double* rs = rec + NS_CHAIN_DOUBLES + NS_TREE_FIXED + 2 * J * 32;
    if (lane < NS_SC) rs[lane] = lane == NS_BASE ? (adapt ? a.par.eps0 : a.par.fixed_eps) : 0.0;
    if (lane < NI_COUNT) ((int*)(rs + NS_SC))[lane] = 0;
    ns_wave_sync();
  }
  s_on[tid] = tid < C ? 1 : 0;
  s_act[tid] = tid;
  int nact = C;
  __syncthreads();

  int bi = 0;                                                   // grid barriers passed
  bool alive = true;
  const long long rounds_max = 1 + (long long)T * ((1ll << J) - 1);
  for (long long round = 0; round < rounds_max; ++round) {
    // ------------------------------------------------------------------------------------------------------------ the pass
    double* mine = a.part + ((size_t)(round & 1) * G + wg) * cstride;
    for (int c0 = 0; c0 < nact; c0 += NS_CT) {
      __syncthreads();
      for (int e = tid; e < NS_CT * 32; e += NS_THREADS) {
        const int c = e >> 5, d = e & 31;
        double v = 0.0;
        if (d < D && c0 + c < nact) v = round == 0 ? sMu[d] : coh_load(a.Theta + (size_t)s_act[c0 + c] * 32 + d);
        sTh[c * HMC_LDW + d] = v;
      }
      double val[4] = {0.0, 0.0, 0.0, 0.0};
      double acc = 0.0;
      for (int64_t row0 = begin; row0 < end; row0 += NS_ROWS) {
        __syncthreads();
        for (int e = tid; e < NS_ROWS * D; e += NS_THREADS) {
          const int rr = e / D, d = e - rr * D;
          sX[rr * HMC_LDW + d] = row0 + rr < end ? a.Z[(size_t)(row0 + rr) * a.ldz + d] : 0.0;
        }
        if (tid < NS_ROWS) {
          const bool in = row0 + tid < end;
          sw[tid] = in ? (a.w ? a.w[row0 + tid] : 1.0) : 0.0;    // (a row past the end: x = 0, w = 0 adds an exact zero)
          sy[tid] = (in && a.family == LAP_POISSON) ? a.Z[(size_t)(row0 + tid) * a.ldz + D] : 0.0;
        }
        __syncthreads();
        {
          const double w = sw[r], y = sy[r];
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            double s = 0.0;
            for (int d = 0; d < D; ++d) s = fma(sX[r * HMC_LDW + d], sTh[(hq + q) * HMC_LDW + d], s);
            double ll, g, h;
            lap_point(a.family, s, y, ll, g, h);
            val[q] += w * ll;
            sG[r * (NS_CT + 1) + hq + q] = w * g;
          }
        }
        __syncthreads();
        if (bd < D) {
          for (int rr = 0; rr < NS_ROWS; ++rr) acc = fma(sG[rr * (NS_CT + 1) + bc], sX[rr * HMC_LDW + bd], acc);
        }
      }
      __syncthreads();
#pragma unroll
      for (int q = 0; q < 4; ++q) sG[tid * 4 + q] = val[q];
      __syncthreads();
      if (bd < D && c0 + bc < nact) coh_store(mine + (size_t)s_act[c0 + bc] * (D + 1) + bd, acc);
      if (tid < NS_CT && c0 + tid < nact) {
        const int base_row = (tid >> 2) * NS_ROWS, q = tid & 3;
        double t = 0.0;
        for (int rr = 0; rr < NS_ROWS; ++rr) t += sG[(base_row + rr) * 4 + q];
        coh_store(mine + (size_t)s_act[c0 + tid] * (D + 1) + D, t);
      }
    }
    ++bi;
    if (!grid_barrier(gs, bi, &s_flag)) { alive = false; break; }

    // ------------------------------------------------------------- the consume, by the owner: its chains to its waves in turn
    // (no workgroup barrier in this loop: the waves take different numbers of chains and different branches)
    for (int c = wg + G * wave; c < C; c += G * NS_WAVES) {
      if (!s_on[c]) continue;
      double* rec = a.recs + (size_t)c * a.rec;
      double* rs = rec + NS_CHAIN_DOUBLES + NS_TREE_FIXED + 2 * J * 32;
      const int tid = lane;                                     // (below, "tid < D" is the wave's lane of a coordinate)
      ns_wave_sync();
      ns_record_io(rec, Sc, Tr, J, false);
      if (tid < NS_SC) s_sc[wave][tid] = rs[tid];
      if (tid < NI_COUNT) s_iv[wave][tid] = ((const int*)(rs + NS_SC))[tid];
      ns_wave_sync();
      if (tid <= D) {                                           // the G records of the chain in workgroup order, then the prior
        const double* all = a.part + (size_t)(round & 1) * G * cstride + (size_t)c * (D + 1) + tid;
        double v = 0.0;
        int g = 0;
        for (; g + 8 <= G; g += 8) {
          double m[8];
#pragma unroll
          for (int u = 0; u < 8; ++u) m[u] = coh_load(all + (size_t)(g + u) * cstride);
#pragma unroll
          for (int u = 0; u < 8; ++u) v += m[u];
        }
        for (; g < G; ++g) v += coh_load(all + (size_t)g * cstride);
        if (tid < D) gth[tid] = v - Sc.th[tid];
        else s_val[wave] = v;
      }
      ns_wave_sync();
      const double logp = s_val[wave] - hmc_half_sq(Sc.th, D);
      double gx = 0.0;
      if (tid < D) for (int i = 0; i < D; ++i) gx = fma(sW[tid * HMC_LDW + i], gth[i], gx);
      double logp_cur = s_sc[wave][NS_LOGP], H0 = s_sc[wave][NS_H0], logW = s_sc[wave][NS_LOGW], logS = s_sc[wave][NS_LOGS], asum = s_sc[wave][NS_ASUM];
      double dsel = s_sc[wave][NS_DSEL], base = s_sc[wave][NS_BASE], hbar = s_sc[wave][NS_HBAR], lebar = s_sc[wave][NS_LEBAR], acc_sum = s_sc[wave][NS_ACC];
      double logp_s = s_sc[wave][NS_LOGPS], h_s = s_sc[wave][NS_HS];
      int ph = s_iv[wave][NI_PH], t = s_iv[wave][NI_T], j = s_iv[wave][NI_J], i = s_iv[wave][NI_I], nleaf = s_iv[wave][NI_NLEAF], depth = s_iv[wave][NI_DEPTH];
      int divergent = s_iv[wave][NI_DIV];
      bool start = false;                                       // a transition starts in this round
      if (ph == 0) {
        // the start state xi = 0: its log target, xi-gradient and theta
        if (tid < D) { Sc.gcur[tid] = gx; Sc.thcur[tid] = Sc.th[tid]; }
        logp_cur = logp;
        if (tid == 0 && !isfinite(logp_cur)) { atomicMax(&a.par.status[0], 2); atomicMax(&a.par.status[1], 2); }
        ph = 1;
        start = true;
      } else {
        const double* z = a.par.noise + ((size_t)c * T + t) * a.noise_ld;
        const double eps = base;
        const bool fwd = z[D + 3 * j] >= 0.0;
        const double v = fwd ? 1.0 : -1.0;
        const double he = v * (0.5 * eps);
        const double* zl = z + D + 3 * J + 2 * ((1 << j) - 1);
        // the leaf's second half kick, its energy and what follows from it
        if (tid < D) {
          Tr.gm[tid] = gx;
          Sc.p[tid] = Sc.p[tid] + he * gx;
        }
        ns_wave_sync();
        const double Hl = hmc_half_sq(Sc.p, D) - logp;
        const double delta = H0 - Hl;
        const bool fin = isfinite(delta);
        asum += fin ? fmin(1.0, exp(delta)) : 0.0;
        ++nleaf;
        if (!fin && tid == 0) { atomicMax(&a.par.status[0], 1); atomicMax(&a.par.status[1], 1); }
        bool ok = true;
        if (!(fin && delta > NUTS_DIVERGENT)) { divergent = 1; ok = false; }
        else {
          bool take = true;
          if (i == 0) {
            logS = delta;
          } else {
            logS = nuts_logaddexp(logS, delta);
            take = logS - delta <= nuts_threshold(zl + 2 * i);
          }
          if (take) {
            if (tid < D) { Tr.xs[tid] = Sc.xp[tid]; Tr.gs[tid] = Tr.gm[tid]; Tr.ths[tid] = Sc.th[tid]; }
            logp_s = logp; h_s = Hl;
          }
          if (i & 1) {
            // the balanced spans that close here: leaves i - 2^m + 1 .. i for every trailing one bit of i
            for (int m = 1; m <= j && ((i >> (m - 1)) & 1); ++m) {
              const int slot = __popc((unsigned)(i - (1 << m) + 1));
              double da = 0.0, db = 0.0;
              for (int q = 0; q < D; ++q) {
                const double d = v * (Sc.xp[q] - Tr.ckx[slot][q]);
                da = fma(d, Tr.ckp[slot][q], da);
                db = fma(d, Sc.p[q], db);
              }
              if (da < 0.0 || db < 0.0) { ok = false; break; }
            }
          } else if (tid < D) {
            const int slot = __popc((unsigned)i);
            Tr.ckx[slot][tid] = Sc.xp[tid];
            Tr.ckp[slot][tid] = Sc.p[tid];
          }
        }
        ns_wave_sync();
        bool tree_done = !ok;                                   // a divergence or a turn inside the doubling: it is discarded, the tree stops
        if (ok) {
          if (i + 1 < (1 << j)) ++i;
          else {
            // the doubling is complete: tree-level selection, the moved endpoint, the tree's own turn test
            const double ej = nuts_threshold(z + D + 3 * j + 1);
            if (logW - logS <= ej) {
              if (tid < D) { Sc.xi[tid] = Tr.xs[tid]; Sc.gcur[tid] = Tr.gs[tid]; Sc.thcur[tid] = Tr.ths[tid]; }
              logp_cur = logp_s;
              dsel = h_s - H0;
            }
            logW = nuts_logaddexp(logW, logS);
            if (tid < D) {
              if (fwd) { Tr.xr[tid] = Sc.xp[tid]; Tr.pr[tid] = Sc.p[tid]; Tr.gr[tid] = Tr.gm[tid]; }
              else { Tr.xl[tid] = Sc.xp[tid]; Tr.pl[tid] = Sc.p[tid]; Tr.gl[tid] = Tr.gm[tid]; }
            }
            depth = j + 1;
            ns_wave_sync();
            double da = 0.0, db = 0.0;
            for (int q = 0; q < D; ++q) {
              const double d = Tr.xr[q] - Tr.xl[q];
              da = fma(d, Tr.pl[q], da);
              db = fma(d, Tr.pr[q], db);
            }
            if (da < 0.0 || db < 0.0 || j + 1 >= J) tree_done = true;
            else { ++j; i = 0; logS = 0.0; logp_s = 0.0; h_s = 0.0; }
          }
        }
        if (tree_done) {
          ns_wave_sync();
          // the new state is the selected one; outputs, adaptation
          const size_t o = (size_t)c * T + t;
          if (tid < ld) {
            a.par.samples[o * ld + tid] = tid < D ? Sc.thcur[tid] : 0.0;
            if (a.par.xis) a.par.xis[o * ld + tid] = tid < D ? Sc.xi[tid] : 0.0;
            if (a.par.props) a.par.props[o * ld + tid] = tid < D ? Sc.xi[tid] : 0.0;
          }
          const double alpha = asum / (double)nleaf;
          if (adapt && t < nwarm) base = hmc_dual_average(t, nwarm, a.par.eps0, alpha, hbar, lebar);
          if (t >= nwarm || nwarm >= T) acc_sum += alpha;
          if (tid == 0) {
            double* dg = a.par.diag + o * NUTS_DIAG;
            dg[0] = alpha; dg[1] = (double)depth; dg[2] = (double)nleaf; dg[3] = base; dg[4] = hbar; dg[5] = lebar;
            dg[6] = divergent ? 1.0 : 0.0; dg[7] = dsel;
            if (t + 1 == T) {
              const int cnt = nwarm >= T ? T : T - nwarm;
              a.par.accept_rate[c] = acc_sum / (double)cnt;
              a.par.eps_final[c] = base;
            }
          }
          ++t;
          start = t < T;
          if (!start) ph = 2;                                   // the chain is done
        }
      }
      if (start) {
        // transition t from its noise row: both endpoints are the state, the first doubling
        const double* z = a.par.noise + ((size_t)c * T + t) * a.noise_ld;
        H0 = hmc_half_sq(z, D) - logp_cur;
        if (tid < D) {
          const double p0 = z[tid], x0 = Sc.xi[tid], g0 = Sc.gcur[tid];
          Tr.xl[tid] = x0; Tr.pl[tid] = p0; Tr.gl[tid] = g0;
          Tr.xr[tid] = x0; Tr.pr[tid] = p0; Tr.gr[tid] = g0;
        }
        logW = 0.0; asum = 0.0; dsel = 0.0; logS = 0.0; logp_s = 0.0; h_s = 0.0;
        nleaf = 0; depth = 0; divergent = 0; j = 0; i = 0;
      }
      if (ph == 1) {
        // the next leaf: from the endpoint its doubling extends when it is the doubling's first; first half kick and drift
        const double* z = a.par.noise + ((size_t)c * T + t) * a.noise_ld;
        const bool fwd = z[D + 3 * j] >= 0.0;
        const double v = fwd ? 1.0 : -1.0;
        const double he = v * (0.5 * base), ve = v * base;
        if (tid < D) {
          if (i == 0) {
            Sc.xp[tid] = fwd ? Tr.xr[tid] : Tr.xl[tid];
            Sc.p[tid] = fwd ? Tr.pr[tid] : Tr.pl[tid];
            Tr.gm[tid] = fwd ? Tr.gr[tid] : Tr.gl[tid];
          }
          const double phf = Sc.p[tid] + he * Tr.gm[tid];
          Sc.p[tid] = phf;
          Sc.xp[tid] = Sc.xp[tid] + ve * phf;
        }
        ns_wave_sync();
        theta();
        ns_wave_sync();
        if (tid < 32) coh_store(a.Theta + (size_t)c * 32 + tid, tid < D ? Sc.th[tid] : 0.0);
      }
      ns_wave_sync();
      ns_record_io(rec, Sc, Tr, J, true);
      if (tid == 0) {
        rs[NS_LOGP] = logp_cur; rs[NS_H0] = H0; rs[NS_LOGW] = logW; rs[NS_LOGS] = logS; rs[NS_ASUM] = asum; rs[NS_DSEL] = dsel;
        rs[NS_BASE] = base; rs[NS_HBAR] = hbar; rs[NS_LEBAR] = lebar; rs[NS_ACC] = acc_sum; rs[NS_LOGPS] = logp_s; rs[NS_HS] = h_s;
        int* ri = (int*)(rs + NS_SC);
        ri[NI_PH] = ph; ri[NI_T] = t; ri[NI_J] = j; ri[NI_I] = i; ri[NI_NLEAF] = nleaf; ri[NI_DEPTH] = depth; ri[NI_DIV] = divergent;
        __hip_atomic_store(a.flags + c, ph == 1 ? 1 : 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
    ++bi;
    if (!grid_barrier(gs, bi, &s_flag)) { alive = false; break; }

    // ------------------------------------------------------------------- the active list, formed alike by every workgroup
    {
      const int f = tid < C ? __hip_atomic_load(a.flags + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0;
      const unsigned long long mask = __ballot(f != 0);
      if (lane == 0) s_cnt[wave] = __popcll(mask);
      __syncthreads();
      int pos = __popcll(mask & ((1ull << lane) - 1ull));
      for (int q = 0; q < wave; ++q) pos += s_cnt[q];
      nact = 0;
      for (int q = 0; q < NS_THREADS / 64; ++q) nact += s_cnt[q];
      s_on[tid] = f != 0;
      if (f != 0) s_act[pos] = tid;
      __syncthreads();
    }
    if (nact == 0) break;
  }
  if (!alive && tid == 0) {                                     // a barrier timed out: every workgroup ends here, after its own bounded wait
    a.par.status[0] = 3;
    atomicMax(&a.par.status[1], 3);
  }
}

static int ns_cap_wgs(int64_t N) {
  const int64_t tiles = (N + NS_ROWS - 1) / NS_ROWS;
  return (int)(tiles < 1 ? 1 : tiles > NS_MAX_WGS ? NS_MAX_WGS : tiles);
}

// the scratch: counter | flags | Theta | records | part
static int64_t ns_flags_offset() { return NS_SYNC_BYTES; }
static int64_t ns_theta_offset() { return ns_flags_offset() + NS_CMAX * (int64_t)sizeof(int); }
static int64_t ns_recs_offset(int32_t C) { return ns_theta_offset() + (int64_t)C * 32 * (int64_t)sizeof(double); }
static int64_t ns_part_offset(int32_t C, int32_t J) { return ns_recs_offset(C) + (int64_t)C * ns_record_doubles(J) * (int64_t)sizeof(double); }

extern "C" int64_t bcx_nuts_stream_scratch_bytes(int64_t N, int32_t D, int32_t chains, int32_t max_depth) {
  if (N < 0 || D < 1 || D > HMC_DMAX || chains < 1 || chains > NS_CMAX || max_depth < 1 || max_depth > NUTS_JMAX) return -1;
  return ns_part_offset(chains, max_depth) + 2 * (int64_t)ns_cap_wgs(N) * chains * (D + 1) * (int64_t)sizeof(double);
}

extern "C" int bcx_nuts_stream(void* stream, int32_t family, int64_t N, int32_t D, const void* w_dev, const void* Z_dev, int64_t ldz,
                               const void* mu_dev, const void* W_dev, int64_t ldw, int32_t chains, int32_t n_warmup, int32_t n_samples,
                               int32_t max_depth, double eps0, double fixed_eps, const void* noise_dev, int64_t noise_ld, int32_t ld,
                               void* samples_dev, void* xi_dev, void* prop_dev, void* diag_dev, void* accept_dev, void* eps_dev,
                               void* status_dev, void* scratch_dev, int64_t scratch_bytes) {
  if (!hmc_common_ok(family, D, chains, n_warmup, n_samples, eps0, ld, noise_dev, samples_dev, diag_dev, accept_dev, eps_dev, status_dev) ||
      N < 0 || chains > NS_CMAX || max_depth < 1 || max_depth > NUTS_JMAX || !scratch_dev || noise_ld < nuts_noise_row(D, max_depth) ||
      (W_dev && ldw < D) || scratch_bytes < bcx_nuts_stream_scratch_bytes(N, D, chains, max_depth) ||
      (N > 0 && (!Z_dev || ldz < D + (family == LAP_POISSON ? 1 : 0))))
    return bcx_fail(BCX_ERR_ARG, "bcx_nuts_stream", "bad arguments (family 0 logistic / 1 Poisson, D <= ld <= 32, at most 256 chains, at least one "
                                                    "transition, max_depth 1 .. 10, noise_ld >= D + 3 max_depth + 2 (2^max_depth - 1), eps0 > 0, ldw >= D, ldz >= D "
                                                    "(Poisson: D + 1), scratch_dev of bcx_nuts_stream_scratch_bytes)");
  static PerDevice<int> resident_of;
  const int resident = one_wg_per_cu((const void*)nuts_stream_kernel, NS_THREADS, resident_of);
  if (resident < 1)
    return bcx_fail(BCX_ERR_STATE, "bcx_nuts_stream", "the kernel's workgroups cannot be resident together on this device");
  const int G = std::max(1, std::min(ns_cap_wgs(N), resident));
  NsArgs a;
  a.par = hmc_par(D, mu_dev, W_dev, ldw, chains, n_warmup, n_samples, 0, eps0, fixed_eps, noise_dev, ld, samples_dev, xi_dev, prop_dev,
                  diag_dev, accept_dev, eps_dev, status_dev);
  char* base = (char*)scratch_dev;
  a.w = (const double*)w_dev; a.Z = (const double*)Z_dev;
  a.flags = (int*)(base + ns_flags_offset()); a.Theta = (double*)(base + ns_theta_offset());
  a.recs = (double*)(base + ns_recs_offset(chains)); a.part = (double*)(base + ns_part_offset(chains, max_depth));
  a.N = N; a.ldz = ldz; a.noise_ld = noise_ld; a.family = family; a.J = max_depth; a.rec = ns_record_doubles(max_depth);
  const GridSync gs = grid_sync_at((unsigned long long*)scratch_dev, 200000000LL);      // 2 s of the 100 MHz wall clock per wait
  hipStream_t st = (hipStream_t)stream;
  BCX_TRY("bcx_nuts_stream", hipMemsetAsync(scratch_dev, 0, NS_SYNC_BYTES, st));
  BCX_TRY("bcx_nuts_stream", hipMemsetAsync(status_dev, 0, sizeof(int), st));
  hipLaunchKernelGGL(nuts_stream_kernel, dim3(G), dim3(NS_THREADS), 0, st, a, gs);
  BCX_TRY("bcx_nuts_stream", hipGetLastError());
  return BCX_OK;
}
