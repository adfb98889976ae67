// cssm_smooth.hip -- the backward launches of cssm_pf_smooth (include/cssm_pf.h).  EXTENSION: forward filtering, backward simulation
// (Godsill, Doucet and West 2004) on the history cssm_pf_interpolate's forward pass keeps, for a cloud of any size: the second user of
// the contract's "backward simulation" (include/cssm_numerics.h) beside k_fleet_backsim (cssm_fleet_smooth.hip).  Every statement is one
// of the contract's functions, an IEEE operation or an exact integer sum, so how slots are mapped to blocks, waves and lanes cannot
// change a bit.
//
// k_fleet_backsim keeps a cloud inside one workgroup and gives a wave a trajectory; at N = 2^20 that leaves a wave per SIMD and sends
// every read of the gathered means through L2.  Here the SLOTS are tiled.  Per time index s, going back, on the handle's stream:
//   k_smooth_tiles<D, 0>  blocks (tile of a.tile slots, group of CSSM_SMOOTH_GROUP trajectories), 256 threads.  The block gathers
//                         mean_c(x_s[i][c]) of its tile once into LDS (D x tile x 8 bytes) and serves every trajectory of its group
//                         from there: a wave owns a trajectory at a time, a lane the slots lane + 64 q of the tile (consecutive
//                         doubles across the wave).  The max of lb over the tile goes to pkey[m][tile] as an order key.
//   k_smooth_fold (LEVEL) a wave per trajectory: level[m] = the max over the tiles' keys.
//   k_smooth_tiles<D, 1>  the same blocks: the exact 128-bit sum of cssm_fix_from_unit(cssm_back_weight(lb, level[m])) over the tile
//                         to psum[m][tile].  The weights are formed again, not kept (n_traj x N doubles).
//   k_smooth_fold (SEARCH) a wave per trajectory: the total, then 64 tiles at a time the running prefix of the tiles' sums until a
//                         tile's end value RN(RN(S_end) / RN(S_tot)) reaches u -- C is non-decreasing, so that tile holds the
//                         contract's first i --, then that tile's slots 64 at a time from the slice; j_s = A_s[i_s] to traj[s][m].
// An index whose record has an sd_c not > 0 (the host decides from the record) runs k_smooth_fold (GEN) alone; a trajectory whose
// level is not > -inf takes the same step inside SEARCH.  Index T is k_smooth_fold (START).  Nothing waits on another block: the passes
// are ordered by the launches; no atomics, no flags; every loop is bounded by the tile, the number of tiles or the group.
//
// k_smooth_rows: k_fleet_lineage's summary (cssm_fleet_rows.hip.h) over the n_traj particles `traj` names in a slice, a block per
// (time index, row) -- the direct source carries nothing from one slice to the next.
#include <hip/hip_runtime.h>

#include "cssm_internal.h"
#include "cssm_kernels.hip.h"
#include "cssm_smooth.hip.h"
#include "cssm_fleet_rows.hip.h"

// record s's transition as the backward kernel reads it: p0, p1 and sd per component, dt
template <int D>
struct SmoothCoef {
  double p0[D], p1[D], sd[D], dt;
  __device__ __forceinline__ SmoothCoef(const StepRec* r, const ModelK& mk) {
    dt = r->dt;
#pragma unroll
    for (int c = 0; c < D; ++c) {
      p0[c] = r->coef[c][0]; p1[c] = r->coef[c][1];
      sd[c] = cssm_back_sd(mk.kind(c), r->coef[c][2], r->coef[c][3]);
    }
  }
};

template <int D, int PASS>
__global__ __launch_bounds__(CSSM_BLOCK) void k_smooth_tiles(const SmoothArgs a) {
  extern __shared__ double s_mean[];                            // [D][tile]: mean_c of the gathered cloud over the block's tile
  const uint32_t n = a.n, M = a.n_traj, tile = a.tile, tid = threadIdx.x, lane = tid & 63u, wid = tid >> 6;
  const uint32_t i0 = blockIdx.x * tile;                        // (< n: the grid has ceil(n / tile) tiles)
  const uint32_t ni = (n - i0 < tile) ? n - i0 : tile;          // the tile's slots
  const uint32_t m0 = blockIdx.y * CSSM_SMOOTH_GROUP;           // (< M: the grid has ceil(M / group) groups)
  const uint32_t cnt = (M - m0 < CSSM_SMOOTH_GROUP) ? M - m0 : CSSM_SMOOTH_GROUP;
  const SmoothCoef<D> k(a.rec, a.mk);
  for (uint32_t li = tid; li < ni; li += CSSM_BLOCK) {
    const uint32_t i = i0 + li, j = a.A ? a.A[i] : i;
#pragma unroll
    for (int c = 0; c < D; ++c) s_mean[(size_t)c * tile + li] = cssm_back_mean(a.mk.kind(c), k.p0[c], k.p1[c], k.dt, a.X[(size_t)c * a.stride + j]);
  }
  __syncthreads();
  const uint32_t* jn_of = a.traj + (size_t)(a.s + 1u) * M;
  for (uint32_t t = wid; t < cnt; t += CSSM_BLOCK / 64) {       // (wave-uniform) the wave's trajectories
    const uint32_t m = m0 + t, jn = jn_of[m];
    double y[D];
#pragma unroll
    for (int c = 0; c < D; ++c) y[c] = a.Xn[(size_t)c * a.stride + jn];
    auto lb_of = [&](uint32_t li) {
      double q = 0.0;
#pragma unroll
      for (int c = 0; c < D; ++c) {
        const double e = (y[c] - s_mean[(size_t)c * tile + li]) / k.sd[c];
        q = q + e * e;
      }
      return cssm_back_lb(q);
    };
    if (PASS == 0) {
      double mx = -cssm_inf();
      for (uint32_t li = lane; li < ni; li += 64u) { const double lb = lb_of(li); mx = (lb > mx) ? lb : mx; }
      const unsigned long long key = wave_max_u64(cssm_order_key(mx));
      if (lane == 0u) a.pkey[(size_t)m * a.ntile + blockIdx.x] = key;
    } else {
      const double level = a.level[m];
      cssm_u128 sa = cssm_u128_zero();
      if (level > -cssm_inf())                                  // (uniform; else the search takes the genealogical step and reads no sum)
        for (uint32_t li = lane; li < ni; li += 64u) sa = cssm_u128_add(sa, cssm_fix_from_unit(cssm_back_weight(lb_of(li), level)));
      const cssm_u128 tot = wave_sum_u128(sa);
      if (lane == 0u) a.psum[(size_t)m * a.ntile + blockIdx.x] = tot;
    }
  }
}

template <int D>
__global__ __launch_bounds__(CSSM_BLOCK) void k_smooth_fold(const SmoothArgs a, const int mode) {
  const uint32_t n = a.n, M = a.n_traj, ntile = a.ntile, s = a.s, lane = threadIdx.x & 63u;
  const uint32_t m = blockIdx.x * (CSSM_BLOCK / 64) + (threadIdx.x >> 6);   // a wave per trajectory
  if (m >= M) return;                                           // (wave-uniform)
  uint32_t* out = a.traj + (size_t)s * M + m;
  if (mode == SMOOTH_START) {
    const uint32_t i = cssm_back_start(m, n, M);
    if (lane == 0u) *out = a.A ? a.A[i] : i;
    return;
  }
  const uint32_t jn = a.traj[(size_t)(s + 1u) * M + m];
  if (mode == SMOOTH_GEN) {
    if (lane == 0u) *out = a.A ? a.A[jn] : jn;
    return;
  }
  if (mode == SMOOTH_LEVEL) {
    unsigned long long key = cssm_order_key(-cssm_inf());
    for (uint32_t tl = lane; tl < ntile; tl += 64u) { const unsigned long long o = a.pkey[(size_t)m * ntile + tl]; key = (o > key) ? o : key; }
    key = wave_max_u64(key);
    if (lane == 0u) a.level[m] = cssm_order_unkey(key);
    return;
  }
  const double level = a.level[m];
  uint32_t is = jn;
  if (level > -cssm_inf()) {                                    // (uniform)
    const cssm_u128* ps = a.psum + (size_t)m * ntile;
    cssm_u128 acc = cssm_u128_zero();
    for (uint32_t tl = lane; tl < ntile; tl += 64u) acc = cssm_u128_add(acc, ps[tl]);
    const cssm_u128 tot = wave_sum_u128(acc);
    const double totd = cssm_u128_to_double(tot);
    const double u = cssm_back_uniform(a.seed, m, s);
    // C is non-decreasing: the first tile whose last slot reaches u holds the crossing (the last tile ends at C = 1 > u)
    cssm_u128 before = cssm_u128_zero();                        // the exact sum of the slots before the tiles (then the slots) at hand
    uint32_t hit_tile = ntile - 1u;
    for (uint32_t base = 0; base < ntile; base += 64u) {        // (uniform) 64 tiles at a time
      const uint32_t tl = base + lane;
      const bool mine = tl < ntile;
      const cssm_u128 v = mine ? ps[tl] : cssm_u128_zero();
      const cssm_u128 inc = cssm_u128_add(before, wave_scan_u128(v, (int)lane));
      const unsigned long long reach = __ballot(mine && cssm_u128_to_double(inc) / totd >= u);
      const bool last = base + 64u >= ntile;
      if (reach || last) {
        const uint32_t L = reach ? (uint32_t)__builtin_ctzll(reach) : ntile - 1u - base;
        const cssm_u128 exc = fleet_u128_sub(inc, v);
        before.lo = readlane_u64(exc.lo, (int)L); before.hi = readlane_u64(exc.hi, (int)L);
        hit_tile = base + L;
        break;
      }
      before.lo = readlane_u64(inc.lo, 63); before.hi = readlane_u64(inc.hi, 63);
    }
    const SmoothCoef<D> k(a.rec, a.mk);
    double y[D];
#pragma unroll
    for (int c = 0; c < D; ++c) y[c] = a.Xn[(size_t)c * a.stride + jn];
    const uint32_t f0 = hit_tile * a.tile;
    const uint32_t f1 = (n - f0 < a.tile) ? n : f0 + a.tile;
    is = f1 - 1u;
    for (uint32_t base = f0; base < f1; base += 64u) {          // (uniform) the tile's slots, 64 at a time, from the slice
      const uint32_t i = base + lane;
      const bool mine = i < f1;
      cssm_u128 F = cssm_u128_zero();
      if (mine) {
        const uint32_t j = a.A ? a.A[i] : i;
        double q = 0.0;
#pragma unroll
        for (int c = 0; c < D; ++c) {
          const double mu = cssm_back_mean(a.mk.kind(c), k.p0[c], k.p1[c], k.dt, a.X[(size_t)c * a.stride + j]);
          const double e = (y[c] - mu) / k.sd[c];
          q = q + e * e;
        }
        F = cssm_fix_from_unit(cssm_back_weight(cssm_back_lb(q), level));
      }
      const cssm_u128 S = cssm_u128_add(before, wave_scan_u128(F, (int)lane));
      const unsigned long long hit = __ballot(mine && cssm_u128_to_double(S) / totd >= u);
      if (hit) { is = base + (uint32_t)__builtin_ctzll(hit); break; }
      before.lo = readlane_u64(S.lo, 63); before.hi = readlane_u64(S.hi, 63);
    }
  }
  if (lane == 0u) *out = a.A ? a.A[is] : is;
}

// Slice s of the handle's history through the particles its trajectories name: fleet_lineage_body's direct source, one slice a block.
template <int D>
struct SmoothSrc {
  static constexpr bool kDirect = true;
  const SmoothRowArgs& a;
  size_t s;
  __device__ __forceinline__ uint32_t ld() const { return (uint32_t)a.stride; }
  __device__ __forceinline__ bool resampled(uint32_t) const { return false; }
  __device__ __forceinline__ const uint32_t* anc(uint32_t) const { return a.traj + s * a.n_traj; }
  __device__ __forceinline__ const double* cloud(uint32_t) const { return a.hist + s * D * a.stride; }
  __device__ __forceinline__ const double* fco(uint32_t) const { return a.fco + s * D; }
  __device__ __forceinline__ double* out(uint32_t) const { return a.out + s * (D + 1) * 3u; }
};

template <int D>
__global__ __launch_bounds__(CSSM_BLOCK) void k_smooth_rows(const SmoothRowArgs a) {
  extern __shared__ unsigned long long s_keys[];
  __shared__ double s_p[CSSM_BLOCK / 64];
  fleet_lineage_body<D>(SmoothSrc<D>{a, (size_t)blockIdx.x}, 1u, a.n_traj, a.np2, blockIdx.y, a.mk, a.lo_state, a.hi_state, a.lo_eta, a.hi_eta,
                        s_keys, nullptr, s_p);
}

// (the launches go through a function template per kernel: DISPATCH_D picks the latent dimension, the template names the instantiation)
template <int D, int PASS>
static int tiles_launch_d(const SmoothLaunch& l) {
  const size_t lds = (size_t)D * l.args.tile * 8u;
  if (lds > 48u * 1024u) {                                      // beyond the default limit of a block's dynamic LDS: asked for by name
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_smooth_tiles<D, PASS>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return (int)e;
  }
  const uint32_t groups = (l.args.n_traj + CSSM_SMOOTH_GROUP - 1u) / CSSM_SMOOTH_GROUP;
  hipLaunchKernelGGL((k_smooth_tiles<D, PASS>), dim3(l.args.ntile, groups), dim3(CSSM_BLOCK), lds, l.stream, l.args);
  return (int)hipGetLastError();
}
template <int D>
static int fold_launch_d(const SmoothLaunch& l, int mode) {
  const uint32_t per = CSSM_BLOCK / 64;
  hipLaunchKernelGGL(k_smooth_fold<D>, dim3((l.args.n_traj + per - 1u) / per), dim3(CSSM_BLOCK), 0, l.stream, l.args, mode);
  return (int)hipGetLastError();
}
template <int D>
static int rows_launch_d(const SmoothRowLaunch& l) {
  hipLaunchKernelGGL(k_smooth_rows<D>, dim3(l.rows, D + 1), dim3(CSSM_BLOCK), (size_t)l.args.np2 * 8u, l.stream, l.args);
  return (int)hipGetLastError();
}

int cssm_smooth_tiles_launch(const SmoothLaunch& l, int pass) {
  int rc = 0;
  if (pass == 0) { DISPATCH_D(l.d, rc = (tiles_launch_d<D, 0>(l))); }
  else { DISPATCH_D(l.d, rc = (tiles_launch_d<D, 1>(l))); }
  return rc;
}

int cssm_smooth_fold_launch(const SmoothLaunch& l, int mode) {
  int rc = 0;
  DISPATCH_D(l.d, rc = fold_launch_d<D>(l, mode));
  return rc;
}

int cssm_smooth_rows_launch(const SmoothRowLaunch& l) {
  int rc = 0;
  DISPATCH_D(l.d, rc = rows_launch_d<D>(l));
  return rc;
}
