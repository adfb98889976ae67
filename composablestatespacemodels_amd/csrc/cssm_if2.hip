// cssm_if2.hip -- cssm_pf_if2 (include/cssm_pf.h): the search of the contract's "iterated filtering" (include/cssm_numerics.h; EXTENSION:
// IF2 of Ionides, Nguyen, Atchade, Stoev and King 2015) for ONE swarm of any size, its particles tiled over many workgroups -- what
// cssm_smooth.hip is to cssm_fleet_smooth.hip.  k_fleet_if2 (cssm_fleet_if2.hip) keeps a swarm's weights and ancestors in one block's LDS
// and so ends at CSSM_FLEET_MAX_N particles; here they live in HBM next to theta[2][n_theta][N] and x[2][d][N].  Every statement is one of
// the contract's functions, an existing device function of the filter, an IEEE operation, an exact integer sum or an integer maximum, so
// how particles are mapped to blocks, waves and lanes cannot change a bit: the result is k_fleet_if2's and the sequential twin's
// (tests/cpp/if2_twin.c).
//
// What needs a grid-wide value is a separate launch (cssm_smooth.hip's rule): no block waits on another inside a kernel -- no flags, no
// spinning, no cooperative launch, no graph; plain launches on the handle's stream, all n_iters x T records enqueued ahead, one
// synchronisation per call.  Per iteration:
//   k_if2_start<D>   a thread per particle: the swarm perturbed at when = 0 into theta buffer 0, x0 from the particle's own m0 and c0,
//                    identity ancestors; ll = 0, ess = N.
//   per record r     k_if2_weigh<D>  a thread per particle: theta and x gathered through the ancestors, perturbed, the particle's own
//                                    coefficients, transition, log-weight into lw; per block the maxima of cssm_order_key(lw) and of the
//                                    level candidates folded into two 64-bit words by integer atomicMax (exact, order-independent).  An
//                                    unweighted record writes identity ancestors and ends here.
//                    k_if2_sums      a block per tile of CSSM_IF2_TILE particles: the level, the weights in place of the log-weights, the
//                                    tile's exact 128-bit sums of cssm_fix_from_unit(w) and of w w into the partials.
//                    k_if2_scan      ONE block: exclusive prefixes of the tiles' sums, the totals, ll, ess, the record's uniform; a
//                                    non-finite max or a zero sum sets the search's dead flag.  It clears the two maxima for the next record.
//                    k_if2_ends      a block per tile: every particle's end slot cnt(C_j) from its exact inclusive prefix (fleet_end_slot).
//                    k_if2_offspring a block per tile of SLOTS: slot s takes the first particle j whose end slot lies beyond s -- the particle
//                                    that owns s in the twin's marker-and-fill statement, because the end slots do not decrease (exact
//                                    sums, monotone roundings, an exact count).  A binary search over the end slots, first narrowed to
//                                    the range the tile's first and last slot give: a particle that owns every slot costs nobody N steps.
//   k_if2_end        blocks (tile, slot of theta): swarm[j][i] = theta[j][anc[i]] and the contract's pairwise tree over the tile in LDS
//                    -- the tile is an aligned power of two, so its levels are the tree's own pairs -- to part[j][tile].
//   k_if2_mean       a block per slot of theta: the same tree continued over the tiles' results; theta_mean, and the iteration's ll.
// Every launch of a dead search returns at its first, uniform, read of the flag.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "cssm_internal.h"
#include "cssm_fleet_if2.hip.h"
#include "cssm_if2_move.hip.h"
#include "cssm_sde_coef.h"

#define CSSM_IF2_ITEMS 4u                                   /* contiguous particles per thread of the tile kernels */
static_assert(CSSM_IF2_TILE == CSSM_BLOCK * CSSM_IF2_ITEMS, "a tile is a block's threads times their items");
static_assert((CSSM_IF2_TILE & (CSSM_IF2_TILE - 1u)) == 0u, "the mean's tree needs an aligned power-of-two tile");

// between the launches of a call
struct If2Ctl {
  unsigned long long kmax, kcmax;    // order keys: the record's max log-weight / max level candidate (0: below every key)
  double totd, u;                    // cssm_u128_to_double(S); the record's resampling uniform
  double ll;
  int32_t ess;
  uint32_t dead;                     // no particle of some record had a usable weight: the search is over
  uint32_t fail_iter;                // ... in this iteration of the call
  uint32_t pad_;
};

struct If2Args {
  uint32_t n, n_theta, ntile, T;
  uint32_t iter;                     // the iteration's row of theta_mean / ll
  uint32_t rec;                      // the record's index
  unsigned long long key;            // cssm_derive_key(seed, first_iter + iter + 1)
  double cool, df;
  double* swarm;                     // [n_theta][n]
  double* theta;                     // [2][n_theta][n], ping-ponged by record parity
  double* x;                         // [2][d][n]
  double* lw;                        // [n]: log-weights, then weights
  uint32_t* anc;                     // [n]
  uint32_t* ends;                    // [n]: end slots
  cssm_u128 *pS, *pS2, *pre;         // [ntile]: the tiles' sums and the exclusive prefixes of pS
  double* part;                      // [n_theta][ntile]: the tiles' results of the mean's tree
  If2Ctl* ctl;
  const unsigned char* recs;         // FleetIf2Rec + d f coefficients each
  const double* rw_sd;
  const double* logtab;
  double* theta_mean;                // [n_iters][n_theta], preset to NaN
  double* ll;                        // [n_iters]
  double* ll_t;                      // may be null
  int32_t* ess_t;                    // may be null
  ModelK mk;
  If2Map map;
};

// the swarm every particle of which starts at theta0
static __global__ __launch_bounds__(CSSM_BLOCK) void k_if2_fill(double* __restrict__ swarm, const double* __restrict__ theta0, uint32_t n) {
  const uint32_t i = blockIdx.x * CSSM_BLOCK + threadIdx.x, j = blockIdx.y;
  if (i < n) swarm[(size_t)j * n + i] = theta0[j];
}

// sd_j cool_m of the perturbation at hand in LDS, padded with zeros (if2_move reads four at a time); ivp slots rest behind x0
__device__ __forceinline__ void if2_stage_sd(const If2Args& a, bool record, double* s_sd) {
  for (uint32_t j = threadIdx.x; j < CSSM_IF2_MAX_THETA + 3u; j += CSSM_BLOCK) {
    const double sdc = (j < a.n_theta) ? a.rw_sd[j] * a.cool : 0.0;
    s_sd[j] = (record && j < a.n_theta && a.map.ivp[j]) ? 0.0 : sdc;
  }
}

template <int D>
__global__ __launch_bounds__(CSSM_BLOCK) void k_if2_start(const If2Args a) {
  __shared__ double s_sd[CSSM_IF2_MAX_THETA + 3];
  if (a.ctl->dead) return;                                      // (uniform)
  const uint32_t n = a.n, i = blockIdx.x * CSSM_BLOCK + threadIdx.x;
  if2_stage_sd(a, false, s_sd);
  const double* tab = stage_log_table(a.logtab);                // (its barrier also completes s_sd)
  if (i < n) {
    if2_move(a.swarm, i, a.theta, i, n, a.n_theta, a.key, 0u, s_sd, tab);
    double z[D];
    draw_normals<D>(a.key, (uint64_t)i, 0u, CSSM_STREAM_INIT, tab, z);
#pragma unroll
    for (int c = 0; c < D; ++c) {
      const int kind = a.mk.kind(c);
      const double m0 = if2_field(a.map, kind, c, CSSM_FIELD_M0, a.theta, i, n), c0 = if2_field(a.map, kind, c, CSSM_FIELD_C0, a.theta, i, n);
      a.x[(size_t)c * n + i] = cssm_sqrt(c0) * z[c] + m0;
    }
    a.anc[i] = i;
  }
  if (i == 0u) { a.ctl->ll = 0.0; a.ctl->ess = (int32_t)n; }
}

template <int D>
__global__ __launch_bounds__(CSSM_BLOCK) void k_if2_weigh(const If2Args a) {
  __shared__ double s_sd[CSSM_IF2_MAX_THETA + 3];
  __shared__ unsigned long long s_wmax[CSSM_BLOCK / 64], s_wref[CSSM_BLOCK / 64];
  if (a.ctl->dead) return;                                      // (uniform)
  const uint32_t n = a.n, nt = a.n_theta, tid = threadIdx.x, i = blockIdx.x * CSSM_BLOCK + tid;
  const unsigned char* g = a.recs + (size_t)a.rec * CSSM_FLEET_IF2_REC_BYTES(D);
  const FleetIf2Rec* h = reinterpret_cast<const FleetIf2Rec*>(g);
  const double* fco = reinterpret_cast<const double*>(g + sizeof(FleetIf2Rec));
  const uint32_t step = h->step;
  const bool weighted = h->has_obs != 0;
  const double dt = h->dt, y = h->y, ypart = h->ypart;
  const int kind_obs = a.mk.obs_kind;
  const bool scaled = kind_obs == CSSM_OBS_GAUSSIAN || kind_obs == CSSM_OBS_NEGBIN || kind_obs == CSSM_OBS_ZIP || kind_obs == CSSM_OBS_STUDENT_T;
  const bool own_level = kind_obs == CSSM_OBS_GAUSSIAN || kind_obs == CSSM_OBS_STUDENT_T;
  const double yk = cssm_obs_y(kind_obs, y);
  const double* tsrc = a.theta + (size_t)(step & 1u) * nt * n;
  double* tdst = a.theta + (size_t)((step & 1u) ^ 1u) * nt * n;
  const double* xsrc = a.x + (size_t)(step & 1u) * D * n;
  double* xdst = a.x + (size_t)((step & 1u) ^ 1u) * D * n;
  if2_stage_sd(a, true, s_sd);
  const double* tab = stage_log_table(a.logtab);
  double tmax = -cssm_inf(), cmax = -cssm_inf();
  if (i < n) {
    const uint32_t j = a.anc[i];
    if2_move(tsrc, j, tdst, i, n, nt, a.key, step + 1u, s_sd, tab);
    double x[D], z[D];
    draw_normals<D>(a.key, (uint64_t)i, step, CSSM_STREAM_STEP, tab, z);
#pragma unroll
    for (int c = 0; c < D; ++c) {
      const int kind = a.mk.kind(c);
      double p[4];
      cssm_sde_coef(kind, if2_field(a.map, kind, c, CSSM_FIELD_MU, tdst, i, n), if2_field(a.map, kind, c, CSSM_FIELD_PHI, tdst, i, n),
                    if2_field(a.map, kind, c, CSSM_FIELD_SIGMA, tdst, i, n), dt, p);
      x[c] = xsrc[(size_t)c * n + j];
      transition_step(kind, p[0], p[1], p[2], p[3], dt, x[c], z[c]);
      xdst[(size_t)c * n + i] = x[c];
    }
    if (weighted) {
      double raw = 0.0, sd = 0.0, cc[4], cdf;
      if (scaled) { raw = tdst[(size_t)a.map.scale_slot * n + i]; sd = cssm_exp(raw); }
      cssm_obs_consts(kind_obs, y, ypart, sd, raw, a.df, cc, &cdf);
      double lw = cssm_obs_logdens(kind_obs, yk, cc, cdf, gamma_coef<D>(a.mk, fco, x));
      if (lw != lw) lw = -cssm_inf();                           // a NaN log-weight is weight zero, not the end of the search
      tmax = lw;
      a.lw[i] = lw;
      if (own_level) cmax = cssm_if2_level(kind_obs, y, sd, a.df);
    } else {
      a.anc[i] = i;                                             // (slot i of anc is read and written by this thread alone)
    }
  }
  if (!weighted) {                                              // (uniform) the cloud and the swarm move, nothing else
    if (i == 0u) {
      if (a.ll_t) a.ll_t[a.rec] = a.ctl->ll;
      if (a.ess_t) a.ess_t[a.rec] = a.ctl->ess;
    }
    return;
  }
  const unsigned long long km = wave_max_u64(cssm_order_key(tmax));
  const unsigned long long kc = wave_max_u64(cssm_order_key(cmax));
  if ((tid & 63u) == 0u) { s_wmax[tid >> 6] = km; s_wref[tid >> 6] = kc; }
  __syncthreads();
  if (tid == 0u) {
    unsigned long long kmax = 0ull, kcmax = 0ull;
    for (uint32_t w = 0; w < CSSM_BLOCK / 64; ++w) { kmax = (s_wmax[w] > kmax) ? s_wmax[w] : kmax; kcmax = (s_wref[w] > kcmax) ? s_wref[w] : kcmax; }
    atomicMax(&a.ctl->kmax, kmax);
    if (own_level) atomicMax(&a.ctl->kcmax, kcmax);
  }
}

// the record's level from the two maxima; false: no particle has a usable weight
__device__ __forceinline__ bool if2_level_of(const If2Args& a, const FleetIf2Rec* h, double* ref) {
  const double gmax = cssm_order_unkey(a.ctl->kmax);
  if (!(gmax > -cssm_inf()) || !(gmax < cssm_inf())) return false;
  const int kind_obs = a.mk.obs_kind;
  const bool own_level = kind_obs == CSSM_OBS_GAUSSIAN || kind_obs == CSSM_OBS_STUDENT_T;
  *ref = cssm_ref_choose(own_level ? cssm_order_unkey(a.ctl->kcmax) : h->ref, gmax);
  return true;
}
__device__ __forceinline__ const FleetIf2Rec* if2_rec_of(const If2Args& a) {
  return reinterpret_cast<const FleetIf2Rec*>(a.recs + (size_t)a.rec * CSSM_FLEET_IF2_REC_BYTES(a.mk.d));
}

// the block's total of a per-thread 128-bit sum (every thread gets it); s_w: a word per wave
__device__ __forceinline__ cssm_u128 if2_block_sum(cssm_u128 v, cssm_u128* s_w) {
  const cssm_u128 w = wave_sum_u128(v);
  if ((threadIdx.x & 63u) == 0u) s_w[threadIdx.x >> 6] = w;
  __syncthreads();
  cssm_u128 tot = cssm_u128_zero();
  for (uint32_t q = 0; q < CSSM_BLOCK / 64; ++q) tot = cssm_u128_add(tot, s_w[q]);
  return tot;
}

static __global__ __launch_bounds__(CSSM_BLOCK) void k_if2_sums(const If2Args a) {
  __shared__ cssm_u128 s_a[CSSM_BLOCK / 64], s_b[CSSM_BLOCK / 64];
  if (a.ctl->dead) return;                                      // (uniform)
  double ref;
  if (!if2_level_of(a, if2_rec_of(a), &ref)) return;            // (uniform) k_if2_scan ends the search
  const uint32_t n = a.n, j0 = blockIdx.x * CSSM_IF2_TILE + threadIdx.x * CSSM_IF2_ITEMS;
  cssm_u128 sa = cssm_u128_zero(), sb = cssm_u128_zero();
#pragma unroll
  for (uint32_t q = 0; q < CSSM_IF2_ITEMS; ++q) {
    const uint32_t j = j0 + q;
    if (j < n) {
      const double w1 = cssm_exp_le0(cssm_min_c(a.lw[j] - ref, CSSM_REF_BELOW));
      a.lw[j] = w1;
      sa = cssm_u128_add(sa, cssm_fix_from_unit(w1));
      sb = cssm_u128_add(sb, cssm_fix_from_unit(w1 * w1));
    }
  }
  const cssm_u128 ta = if2_block_sum(sa, s_a), tb = if2_block_sum(sb, s_b);
  if (threadIdx.x == 0u) { a.pS[blockIdx.x] = ta; a.pS2[blockIdx.x] = tb; }
}

static __global__ __launch_bounds__(CSSM_BLOCK) void k_if2_scan(const If2Args a) {
  __shared__ cssm_u128 s_wS[CSSM_BLOCK / 64], s_wS2[CSSM_BLOCK / 64];
  If2Ctl* ctl = a.ctl;
  if (ctl->dead) return;                                        // (uniform)
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wid = tid >> 6, ntile = a.ntile;
  const FleetIf2Rec* h = if2_rec_of(a);
  double ref;
  const bool usable = if2_level_of(a, h, &ref);
  __syncthreads();                                              // every thread has read the maxima and the flag
  if (!usable) {                                                // (uniform)
    if (tid == 0u) { ctl->dead = 1u; ctl->fail_iter = a.iter; }
    return;
  }
  const uint32_t it = (ntile + CSSM_BLOCK - 1u) / CSSM_BLOCK;   // tiles per thread (contiguous)
  const uint32_t b0 = (tid * it < ntile) ? tid * it : ntile;
  const uint32_t b1 = (b0 + it < ntile) ? b0 + it : ntile;
  cssm_u128 sa = cssm_u128_zero(), sb = cssm_u128_zero();
  for (uint32_t b = b0; b < b1; ++b) { sa = cssm_u128_add(sa, a.pS[b]); sb = cssm_u128_add(sb, a.pS2[b]); }
  const cssm_u128 inc = wave_scan_u128(sa, (int)lane);
  const cssm_u128 wb2 = wave_sum_u128(sb);
  if (lane == 63u) { s_wS[wid] = inc; s_wS2[wid] = wb2; }
  __syncthreads();
  cssm_u128 tot = cssm_u128_zero(), tot2 = cssm_u128_zero(), off = cssm_u128_zero();
  for (uint32_t w = 0; w < CSSM_BLOCK / 64; ++w) {
    if (w < wid) off = cssm_u128_add(off, s_wS[w]);
    tot = cssm_u128_add(tot, s_wS[w]); tot2 = cssm_u128_add(tot2, s_wS2[w]);
  }
  if (cssm_u128_is_zero(tot)) {                                 // (uniform)
    if (tid == 0u) { ctl->dead = 1u; ctl->fail_iter = a.iter; }
    return;
  }
  cssm_u128 run = fleet_u128_sub(cssm_u128_add(off, inc), sa);
  for (uint32_t b = b0; b < b1; ++b) { a.pre[b] = run; run = cssm_u128_add(run, a.pS[b]); }
  if (tid == 0u) {
    const double ll = ctl->ll + ref + cssm_log(cssm_fix_to_double(tot) / (double)a.n);
    const int32_t ess = cssm_ess_of(tot, tot2);
    ctl->ll = ll; ctl->ess = ess;
    ctl->totd = cssm_u128_to_double(tot); ctl->u = cssm_if2_uniform(a.key, h->step);
    ctl->kmax = 0ull; ctl->kcmax = 0ull;                        // the next weighted record's maxima start below every key
    if (a.ll_t) a.ll_t[a.rec] = ll;
    if (a.ess_t) a.ess_t[a.rec] = ess;
  }
}

static __global__ __launch_bounds__(CSSM_BLOCK) void k_if2_ends(const If2Args a) {
  __shared__ cssm_u128 s_w[CSSM_BLOCK / 64];
  if (a.ctl->dead) return;                                      // (uniform)
  const uint32_t n = a.n, tid = threadIdx.x, lane = tid & 63u, wid = tid >> 6;
  const uint32_t j0 = blockIdx.x * CSSM_IF2_TILE + tid * CSSM_IF2_ITEMS;
  const double totd = a.ctl->totd, u = a.ctl->u, inv_n = 1.0 / (double)n;
  const bool pow2 = (n & (n - 1u)) == 0u;
  cssm_u128 f[CSSM_IF2_ITEMS], sa = cssm_u128_zero();
#pragma unroll
  for (uint32_t q = 0; q < CSSM_IF2_ITEMS; ++q) {
    f[q] = (j0 + q < n) ? cssm_fix_from_unit(a.lw[j0 + q]) : cssm_u128_zero();
    sa = cssm_u128_add(sa, f[q]);
  }
  const cssm_u128 inc = wave_scan_u128(sa, (int)lane);
  if (lane == 63u) s_w[wid] = inc;
  __syncthreads();
  cssm_u128 run = a.pre[blockIdx.x];
  for (uint32_t w = 0; w < wid; ++w) run = cssm_u128_add(run, s_w[w]);
  run = fleet_u128_sub(cssm_u128_add(run, inc), sa);
#pragma unroll
  for (uint32_t q = 0; q < CSSM_IF2_ITEMS; ++q) {
    run = cssm_u128_add(run, f[q]);
    if (j0 + q < n) a.ends[j0 + q] = fleet_end_slot(run, totd, u, n, pow2, inv_n);
  }
}

// the first j in [lo, hi] whose end slot lies beyond s; ends[hi] > s is the caller's (every index read lies in [lo, hi])
__device__ __forceinline__ uint32_t if2_owner(const uint32_t* __restrict__ ends, uint32_t s, uint32_t lo, uint32_t hi) {
  while (lo < hi) {                                             // at most 32 rounds
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (ends[mid] > s) hi = mid; else lo = mid + 1u;
  }
  return lo;
}

static __global__ __launch_bounds__(CSSM_BLOCK) void k_if2_offspring(const If2Args a) {
  __shared__ uint32_t s_lo, s_hi;
  if (a.ctl->dead) return;                                      // (uniform)
  const uint32_t n = a.n, tid = threadIdx.x;
  const uint32_t s0 = blockIdx.x * CSSM_IF2_TILE;               // (< n: the grid has ceil(n / tile) tiles)
  const uint32_t s1 = (n - s0 < CSSM_IF2_TILE) ? n : s0 + CSSM_IF2_TILE;
  // ends[n - 1] = n (C = 1 counts every grid point), so every slot has an owner in [0, n - 1]
  if (tid == 0u) s_lo = if2_owner(a.ends, s0, 0u, n - 1u);
  if (tid == 64u) s_hi = if2_owner(a.ends, s1 - 1u, 0u, n - 1u);
  __syncthreads();
  const uint32_t lo = s_lo, hi = s_hi;
  for (uint32_t s = s0 + tid; s < s1; s += CSSM_BLOCK) a.anc[s] = if2_owner(a.ends, s, lo, hi);
}

static __global__ __launch_bounds__(CSSM_BLOCK) void k_if2_end(const If2Args a) {
  __shared__ double s_v[CSSM_IF2_TILE];
  if (a.ctl->dead) return;                                      // (uniform)
  const uint32_t n = a.n, tid = threadIdx.x, j = blockIdx.y, i0 = blockIdx.x * CSSM_IF2_TILE;
  const double* tfin = a.theta + ((size_t)(a.T & 1u) * a.n_theta + j) * n;   // record T - 1 wrote buffer T & 1
  double* sw = a.swarm + (size_t)j * n;
  for (uint32_t li = tid; li < CSSM_IF2_TILE; li += CSSM_BLOCK) {
    const uint32_t i = i0 + li;
    if (i < n) {
      const double v = tfin[a.anc[i]];
      sw[i] = v;
      s_v[li] = v;
    }
  }
  // level l pairs the elements at i 2^(l+1) and i 2^(l+1) + 2^l of the WHOLE index: i0 is a multiple of the tile, so the pairs are the tile's
  for (uint32_t stride = 1u; stride < CSSM_IF2_TILE && stride < n; stride <<= 1) {
    __syncthreads();
    for (uint32_t li = tid * 2u * stride; li < CSSM_IF2_TILE; li += CSSM_BLOCK * 2u * stride)
      if (i0 + li < n) s_v[li] = s_v[li] + ((i0 + li + stride < n) ? s_v[li + stride] : 0.0);   // (an absent partner adds + 0.0, as the twin states it)
  }
  __syncthreads();
  if (tid == 0u) a.part[(size_t)j * a.ntile + blockIdx.x] = s_v[0];
}

static __global__ __launch_bounds__(CSSM_BLOCK) void k_if2_mean(const If2Args a) {
  if (a.ctl->dead) return;                                      // (uniform)
  const uint32_t tid = threadIdx.x, j = blockIdx.x, ntile = a.ntile;
  double* row = a.part + (size_t)j * ntile;                     // this block's alone
  for (uint32_t stride = 1u; stride < ntile; stride <<= 1) {    // the tree goes on over the tiles: tile b stands at index b CSSM_IF2_TILE
    __syncthreads();
    for (uint32_t b = tid * 2u * stride; b < ntile; b += CSSM_BLOCK * 2u * stride)
      row[b] = row[b] + ((b + stride < ntile) ? row[b + stride] : 0.0);
  }
  __syncthreads();
  if (tid == 0u) {
    a.theta_mean[(size_t)a.iter * a.n_theta + j] = row[0] / (double)a.n;
    if (j == 0u) a.ll[a.iter] = a.ctl->ll;
  }
}

template <int D>
static void if2_launch_start_d(const If2Args& a, uint32_t blocks, hipStream_t st) { hipLaunchKernelGGL(k_if2_start<D>, dim3(blocks), dim3(CSSM_BLOCK), 0, st, a); }
template <int D>
static void if2_launch_weigh_d(const If2Args& a, uint32_t blocks, hipStream_t st) { hipLaunchKernelGGL(k_if2_weigh<D>, dim3(blocks), dim3(CSSM_BLOCK), 0, st, a); }

extern "C" int cssm_pf_if2(cssm_pf* pf, const double* theta0, const double* swarm0, size_t n_theta, const double* rw_sd, double cooling_fraction_50,
                           uint32_t first_iter, uint32_t n_iters, uint64_t seed, const double* t, const double* y, const uint8_t* has_obs, size_t T,
                           double* theta_mean, double* ll, double* swarm_out, double* ll_t, int32_t* ess_t, double* x_out, uint32_t* anc_out) {
  if (!rw_sd) return fail(CSSM_EINVAL_ARG, "cssm_pf_if2: rw_sd is null");
  if (!theta_mean || !ll) return fail(CSSM_EINVAL_ARG, "cssm_pf_if2: null output (theta_mean, ll)");
  if (T > 0 && (!t || !y)) return fail(CSSM_EINVAL_ARG, "cssm_pf_if2: null data (t, y) with T = %zu", T);
  if (T > 0xfffffffeull) return fail(CSSM_EINVAL_ARG, "cssm_pf_if2: too many records");
  if (!theta0 && !swarm0) return fail(CSSM_EINVAL_ARG, "cssm_pf_if2: theta0 and swarm0 are both null (a starting row, or a whole swarm)");
  if (n_theta > CSSM_IF2_MAX_THETA) return fail(CSSM_EINVAL_ARG, "cssm_pf_if2: n_theta = %zu exceeds CSSM_IF2_MAX_THETA = %d", n_theta, CSSM_IF2_MAX_THETA);
  for (size_t j = 0; j < n_theta; ++j)
    if (!(rw_sd[j] >= 0.0) || !std::isfinite(rw_sd[j]))
      return fail(CSSM_EINVAL_ARG, "cssm_pf_if2: rw_sd[%zu] = %g must be finite and not negative (0 keeps the slot fixed)", j, rw_sd[j]);
  if (n_iters < 1u || n_iters > 1000000u) return fail(CSSM_EINVAL_ARG, "cssm_pf_if2: n_iters must be in [1, 1000000] (got %u)", n_iters);
  if ((uint64_t)first_iter + n_iters > (1ull << 31)) return fail(CSSM_EINVAL_ARG, "cssm_pf_if2: first_iter + n_iters must not exceed 2^31");
  if (!(cooling_fraction_50 > 0.0 && cooling_fraction_50 <= 1.0))
    return fail(CSSM_EINVAL_ARG, "cssm_pf_if2: cooling_fraction_50 = %g must be in (0, 1] (the factor the random walk shrinks by over 50 iterations)",
                cooling_fraction_50);
  if (!pf) return fail(CSSM_EINVAL_ARG, "cssm_pf_if2: null handle");
  // ---- the handle
  if (pf->obs_kind == CSSM_OBS_LGCP)
    return fail(CSSM_EINVAL_ARG, "cssm_pf_if2: an LGCP handle is not served (the contract's search weighs one density per record, not a chain of sub-steps)");
  if (pf->sharded) return fail(CSSM_ESTATE, "cssm_pf_if2 runs on a single-GPU handle");
  if (pf->resampler != CSSM_RESAMPLE_SYSTEMATIC)
    return fail(CSSM_ESTATE, "cssm_pf_if2: the handle's CSSM_OPT_RESAMPLER is %d; the contract's search resamples systematically (CSSM_RESAMPLE_SYSTEMATIC)",
                pf->resampler);
  if (!pf->if2_map_ok || (size_t)pf->if2_map.n_theta != n_theta)
    return fail(CSSM_EINVAL_ARG, "cssm_pf_if2: n_theta = %zu, the handle's descriptor flattens to %d (cssm_desc_flatten)", n_theta,
                pf->if2_map_ok ? (int)pf->if2_map.n_theta : -1);
  if (pf->n > 0xffffffffull - CSSM_IF2_TILE) return fail(CSSM_EINVAL_ARG, "cssm_pf_if2: too many particles");
  std::vector<double> cool(n_iters);
  if (const int crc = cssm_fleet_if2_cooling(cooling_fraction_50, first_iter, n_iters, cool.data())) return crc;
  HIP_TRY(hipSetDevice(pf->device));
  const uint32_t n = (uint32_t)pf->n, nt = (uint32_t)n_theta, ntile = (n + CSSM_IF2_TILE - 1u) / CSSM_IF2_TILE, nblk = (n + CSSM_BLOCK - 1u) / CSSM_BLOCK;
  const int d = pf->d;
  const size_t RB = CSSM_FLEET_IF2_REC_BYTES(d);
  // staged upload: rw_sd | theta0 | records
  const size_t o_th = (size_t)CSSM_IF2_MAX_THETA * 8u, o_recs = 2u * o_th;
  std::vector<unsigned char> stage(o_recs + T * RB + 8u, 0);
  memcpy(stage.data(), rw_sd, (size_t)nt * 8u);
  if (theta0) memcpy(stage.data() + o_th, theta0, (size_t)nt * 8u);
  {
    const bool own_level = pf->obs_kind == CSSM_OBS_GAUSSIAN || pf->obs_kind == CSSM_OBS_STUDENT_T;
    double tp = T ? cssm_series_t0(t, T) : 0.0;
    for (size_t s = 0; s < T; ++s) {                             // what of a record does not depend on the parameters (fleet_if2_recs)
      StepRec rec;
      cssm_build_rec(pf, tp, t[s], y[s], has_obs ? (int)has_obs[s] : 1, (uint32_t)s, &rec);
      FleetIf2Rec h;
      h.y = y[s]; h.ypart = cssm_obs_ypart(pf->obs_kind, y[s], (double)pf->obs_df);
      h.ref = own_level ? 0.0 : cssm_if2_level(pf->obs_kind, y[s], 1.0, (double)pf->obs_df);
      h.dt = rec.dt; h.has_obs = rec.has_obs; h.step = rec.step;
      unsigned char* dst = stage.data() + o_recs + s * RB;
      memcpy(dst, &h, sizeof h);
      memcpy(dst + sizeof h, rec.fco, (size_t)d * 8u);
      tp = t[s];
    }
  }
  // the work space first: a refusal here finds the handle as it was
  CssmTemps tmp;
  unsigned char* d_stage = nullptr;
  double *d_swarm = nullptr, *d_theta = nullptr, *d_x = nullptr, *d_lw = nullptr, *d_part = nullptr, *d_mean = nullptr, *d_ll = nullptr, *d_ll_t = nullptr;
  int32_t* d_ess_t = nullptr; uint32_t *d_anc = nullptr, *d_ends = nullptr; cssm_u128* d_sums = nullptr; If2Ctl* d_ctl = nullptr;
  const size_t sw_bytes = (size_t)nt * n * 8u, x_bytes = 2u * (size_t)d * n * 8u, mean_bytes = (size_t)n_iters * nt * 8u;
  const size_t work = stage.size() + 3u * sw_bytes + x_bytes + (size_t)n * 16u + (size_t)ntile * (48u + 8u * nt) + mean_bytes + (size_t)n_iters * 8u +
                      T * 12u + sizeof(If2Ctl);
  if (tmp.alloc(d_stage, stage.size()) != hipSuccess || tmp.alloc(d_swarm, std::max<size_t>(sw_bytes, 8u)) != hipSuccess ||
      tmp.alloc(d_theta, std::max<size_t>(2u * sw_bytes, 8u)) != hipSuccess || tmp.alloc(d_x, x_bytes) != hipSuccess ||
      tmp.alloc(d_lw, (size_t)n * 8u) != hipSuccess || tmp.alloc(d_anc, (size_t)n * 4u) != hipSuccess || tmp.alloc(d_ends, (size_t)n * 4u) != hipSuccess ||
      tmp.alloc(d_sums, (size_t)ntile * 48u) != hipSuccess || tmp.alloc(d_part, std::max<size_t>((size_t)ntile * nt * 8u, 8u)) != hipSuccess ||
      tmp.alloc(d_mean, std::max<size_t>(mean_bytes, 8u)) != hipSuccess || tmp.alloc(d_ll, (size_t)n_iters * 8u) != hipSuccess ||
      tmp.alloc(d_ll_t, (T + 1u) * 8u) != hipSuccess || tmp.alloc(d_ess_t, (T + 1u) * 4u) != hipSuccess || tmp.alloc(d_ctl, sizeof(If2Ctl)) != hipSuccess)
    return fail(CSSM_ENOMEM, "cssm_pf_if2: the swarm, the states and the partials of the search do not fit (%zu bytes)", work);
  hipEvent_t e0 = nullptr, e1 = nullptr;
  HIP_TRY(tmp.event(e0)); HIP_TRY(tmp.event(e1));
  HIP_TRY(hipMemcpyAsync(d_stage, stage.data(), stage.size(), hipMemcpyHostToDevice, pf->stream));
  if (swarm0 && sw_bytes) HIP_TRY(hipMemcpyAsync(d_swarm, swarm0, sw_bytes, hipMemcpyHostToDevice, pf->stream));
  HIP_TRY(hipStreamSynchronize(pf->stream));                    // (stage and swarm0 are pageable)
  HIP_TRY(hipMemsetAsync(d_ctl, 0, sizeof(If2Ctl), pf->stream));
  HIP_TRY(hipMemsetAsync(d_mean, 0xff, std::max<size_t>(mean_bytes, 8u), pf->stream));   // (rows no iteration writes are not read back)
  HIP_TRY(hipMemsetAsync(d_ll, 0xff, (size_t)n_iters * 8u, pf->stream));
  If2Args a{};
  a.n = n; a.n_theta = nt; a.ntile = ntile; a.T = (uint32_t)T;
  a.df = (double)pf->obs_df;
  a.swarm = d_swarm; a.theta = d_theta; a.x = d_x; a.lw = d_lw; a.anc = d_anc; a.ends = d_ends;
  a.pS = d_sums; a.pS2 = d_sums + ntile; a.pre = d_sums + 2u * (size_t)ntile; a.part = d_part; a.ctl = d_ctl;
  a.recs = d_stage + o_recs; a.rw_sd = reinterpret_cast<const double*>(d_stage); a.logtab = pf->d_logtab;
  a.theta_mean = d_mean; a.ll = d_ll; a.ll_t = ll_t ? d_ll_t : nullptr; a.ess_t = ess_t ? d_ess_t : nullptr;
  a.mk = pf->mk; a.map = pf->if2_map;
  HIP_TRY(hipEventRecord(e0, pf->stream));
  if (!swarm0 && nt) {
    hipLaunchKernelGGL(k_if2_fill, dim3(nblk, nt), dim3(CSSM_BLOCK), 0, pf->stream, d_swarm, reinterpret_cast<const double*>(d_stage + o_th), n);
    HIP_TRY(hipGetLastError());
  }
  for (uint32_t q = 0; q < n_iters && T; ++q) {
    a.iter = q; a.cool = cool[q]; a.key = cssm_derive_key(seed, (uint64_t)first_iter + q + 1u);
    DISPATCH_D(d, if2_launch_start_d<D>(a, nblk, pf->stream));
    HIP_TRY(hipGetLastError());
    for (size_t r = 0; r < T; ++r) {
      a.rec = (uint32_t)r;
      DISPATCH_D(d, if2_launch_weigh_d<D>(a, nblk, pf->stream));
      if (!(has_obs ? has_obs[r] != 0 : true)) continue;
      hipLaunchKernelGGL(k_if2_sums, dim3(ntile), dim3(CSSM_BLOCK), 0, pf->stream, a);
      hipLaunchKernelGGL(k_if2_scan, dim3(1), dim3(CSSM_BLOCK), 0, pf->stream, a);
      hipLaunchKernelGGL(k_if2_ends, dim3(ntile), dim3(CSSM_BLOCK), 0, pf->stream, a);
      hipLaunchKernelGGL(k_if2_offspring, dim3(ntile), dim3(CSSM_BLOCK), 0, pf->stream, a);
      HIP_TRY(hipGetLastError());
    }
    if (nt) {
      hipLaunchKernelGGL(k_if2_end, dim3(ntile, nt), dim3(CSSM_BLOCK), 0, pf->stream, a);
      hipLaunchKernelGGL(k_if2_mean, dim3(nt), dim3(CSSM_BLOCK), 0, pf->stream, a);
    }
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipEventRecord(e1, pf->stream));
  std::vector<double> h_mean((size_t)n_iters * nt), h_ll(n_iters);
  If2Ctl h_ctl;
  if (mean_bytes) HIP_TRY(hipMemcpyAsync(h_mean.data(), d_mean, mean_bytes, hipMemcpyDeviceToHost, pf->stream));
  HIP_TRY(hipMemcpyAsync(h_ll.data(), d_ll, (size_t)n_iters * 8u, hipMemcpyDeviceToHost, pf->stream));
  HIP_TRY(hipMemcpyAsync(&h_ctl, d_ctl, sizeof h_ctl, hipMemcpyDeviceToHost, pf->stream));
  if (swarm_out && sw_bytes) HIP_TRY(hipMemcpyAsync(swarm_out, d_swarm, sw_bytes, hipMemcpyDeviceToHost, pf->stream));
  if (ll_t && T) HIP_TRY(hipMemcpyAsync(ll_t, d_ll_t, T * 8u, hipMemcpyDeviceToHost, pf->stream));
  if (ess_t && T) HIP_TRY(hipMemcpyAsync(ess_t, d_ess_t, T * 4u, hipMemcpyDeviceToHost, pf->stream));
  if (x_out) HIP_TRY(hipMemcpyAsync(x_out, d_x + (size_t)(T & 1u) * d * n, (size_t)d * n * 8u, hipMemcpyDeviceToHost, pf->stream));   // record T - 1 wrote buffer T & 1
  if (anc_out) HIP_TRY(hipMemcpyAsync(anc_out, d_anc, (size_t)n * 4u, hipMemcpyDeviceToHost, pf->stream));
  HIP_TRY(hipStreamSynchronize(pf->stream));
  float ms = 0.f;
  pf->if2_ms = (hipEventElapsedTime(&ms, e0, e1) == hipSuccess) ? (double)ms : 0.0;
  const bool failed = T != 0 && h_ctl.dead != 0u;
  const uint32_t done = T == 0 ? 0u : (failed ? h_ctl.fail_iter : n_iters);   // the iterations whose rows stand
  for (uint32_t m = 0; m < n_iters; ++m) {
    ll[m] = m < done ? h_ll[m] : cssm_nan();
    for (size_t j = 0; j < nt; ++j) theta_mean[(size_t)m * nt + j] = m < done ? h_mean[(size_t)m * nt + j] : cssm_nan();
  }
  const bool whole = T != 0 && !failed;                          // the last iteration's diagnostics exist
  if (ll_t && !whole) std::fill(ll_t, ll_t + T, cssm_nan());
  if (ess_t && !whole) std::fill(ess_t, ess_t + T, -1);
  if (anc_out && !whole) std::fill(anc_out, anc_out + n, 0xffffffffu);
  if (x_out && !whole) std::fill(x_out, x_out + (size_t)d * n, cssm_nan());
  if (failed) return fail(CSSM_ENONFINITE, "cssm_pf_if2: a record of iteration %u left no particle a usable weight (the search ended there)", h_ctl.fail_iter);
  return CSSM_OK;
}

extern "C" int cssm_pf_if2_last_ms(cssm_pf* pf, double* ms) {
  if (!pf || !ms) return fail(CSSM_EINVAL_ARG, "null argument");
  if (pf->if2_ms < 0.0) return fail(CSSM_ESTATE, "no search has run on this handle (cssm_pf_if2 first)");
  *ms = pf->if2_ms;
  return CSSM_OK;
}
