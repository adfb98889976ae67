// cssm_fleet_smooth.hip -- the two backward launches of cssm_fleet_smooth (include/cssm_pf.h).  EXTENSION: forward filtering, backward
// simulation (Godsill, Doucet and West 2004); the reference has no smoother beyond FilterInterpolate.  The arithmetic is the contract's
// (include/cssm_numerics.h, "backward simulation"): every statement here is one of its functions, an IEEE operation or an exact integer
// sum, so how slots are mapped to lanes and where the cloud is read from cannot change a bit.
//
// k_fleet_backsim: blocks (series b of the chunk, group g of CSSM_BACKSIM_TPB trajectories), 256 threads.  The block walks the time
// indices from T - 1 back to 0 in lock step; per index it gathers mean_c(x_s[i][c]) of every slot once -- the part of the backward
// kernel that does not depend on the trajectory -- into LDS (STAGE) or forms it again from the slice through L2 where d N 8 bytes do
// not fit.  A wave owns one trajectory at a time (trajectory t of the group belongs to wave t & 3), a lane a contiguous range of
// ceil(N / 64) slots: pass 1 the level (wave_max_u64), pass 2 the weights' fixed-point sums (wave_scan_u128), then the lane whose range
// holds the crossing is known and its slots are evaluated once more, one per lane.  The weights are formed twice rather than kept:
// N doubles per wave do not fit beside the staged means at N = 4096.  Up to CSSM_BACKSIM_STAGE_MAX bytes are staged (d = 3 at N = 4096:
// 96 KiB, one block per CU); beyond 48 KiB the launch asks for the dynamic LDS by name.  Nothing crosses a block: no atomics, no flags, every loop is
// bounded by N, T_k or the group's size.
//
// k_fleet_smooth_rows: k_fleet_lineage's summary (cssm_fleet_rows.hip.h) over the M particles `traj` names per slice.
#include <hip/hip_runtime.h>

#include "cssm_internal.h"
#include "cssm_kernels.hip.h"
#include "cssm_fleet_smooth.hip.h"
#include "cssm_fleet_rows.hip.h"

template <int D, bool STAGE>
__global__ __launch_bounds__(CSSM_BLOCK) void k_fleet_backsim(const FleetBackArgs a) {
  extern __shared__ double s_mean[];                            // (STAGE) [D][n]: mean_c of the gathered cloud of the index at hand
  __shared__ uint32_t s_j[CSSM_BACKSIM_TPB];                    // j_{s+1} of the group's trajectories
  const uint32_t n = a.n, M = a.n_traj, b = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wid = tid >> 6;
  const unsigned long long r0 = a.off[b], r1 = a.off[b + 1];
  const uint32_t T = (uint32_t)(r1 - r0);
  if (T == 0u || a.ser[b].err != 0u) return;                    // (uniform) no records, or the forward pass gave the series up
  const uint32_t m0 = blockIdx.y * CSSM_BACKSIM_TPB;
  if (m0 >= M) return;                                          // (uniform)
  const uint32_t cnt = (M - m0 < CSSM_BACKSIM_TPB) ? M - m0 : CSSM_BACKSIM_TPB;
  const size_t base = (size_t)r0 + b;                           // the series' first slice
  const uint64_t seed = a.par[a.k0 + b].seed;
  constexpr uint32_t RB = (uint32_t)CSSM_FLEET_REC_BYTES(D);
  auto head_of = [&](uint32_t s) { return reinterpret_cast<const FleetRecHead*>(a.recs + ((size_t)r0 + s) * RB); };
  {                                                             // index T: slot floor(m N / M) of the final filtering cloud
    const bool res = head_of(T - 1u)->has_obs != 0;
    const uint32_t* A = a.hanc + (base + T) * n;
    for (uint32_t t = tid; t < cnt; t += CSSM_BLOCK) {
      const uint32_t i = cssm_back_start(m0 + t, n, M);
      const uint32_t j = res ? A[i] : i;
      s_j[t] = j;
      a.traj[(base + T) * M + m0 + t] = j;
    }
  }
  const uint32_t it = (n + 63u) >> 6;                           // slots per lane (contiguous)
  const uint32_t i0 = (lane * it < n) ? lane * it : n;
  const uint32_t i1 = (i0 + it < n) ? i0 + it : n;
  for (uint32_t s = T; s-- > 0u;) {                             // bounded by the series' length
    __syncthreads();                                            // s_j of the index behind is complete; s_mean is free
    const FleetRecHead* h = head_of(s);
    const double* tail = reinterpret_cast<const double*>(reinterpret_cast<const unsigned char*>(h) + sizeof(FleetRecHead));
    const double dt = h->dt;
    const bool res = s >= 1u && head_of(s - 1u)->has_obs != 0;  // A_s exists (else the identity)
    const uint32_t* A = a.hanc + (base + s) * n;
    const double* X = a.hist + (base + s) * D * n;
    const double* Xn = a.hist + (base + s + 1u) * D * n;
    double p0[D], p1[D], sd[D];
    bool gen = false;                                           // (uniform) the genealogical step
#pragma unroll
    for (int c = 0; c < D; ++c) {
      p0[c] = tail[4 * c]; p1[c] = tail[4 * c + 1];
      sd[c] = cssm_back_sd(a.mk.kind(c), tail[4 * c + 2], tail[4 * c + 3]);
      if (!(sd[c] > 0.0)) gen = true;
    }
    auto mean_of = [&](uint32_t i, int c) {                     // mean_c(x_s[i][c]) from the slice
      const uint32_t j = res ? A[i] : i;
      return cssm_back_mean(a.mk.kind(c), p0[c], p1[c], dt, X[(size_t)c * n + j]);
    };
    if (STAGE && !gen) {
      for (uint32_t i = tid; i < n; i += CSSM_BLOCK) {
#pragma unroll
        for (int c = 0; c < D; ++c) s_mean[(size_t)c * n + i] = mean_of(i, c);
      }
    }
    __syncthreads();
    for (uint32_t t = wid; t < cnt; t += CSSM_BLOCK / 64) {     // (wave-uniform) the wave's trajectories
      const uint32_t m = m0 + t, jn = s_j[t];
      uint32_t is = jn;
      if (!gen) {
        double y[D];
#pragma unroll
        for (int c = 0; c < D; ++c) y[c] = Xn[(size_t)c * n + jn];
        auto lb_of = [&](uint32_t i) {
          double q = 0.0;
#pragma unroll
          for (int c = 0; c < D; ++c) {
            const double mu = STAGE ? s_mean[(size_t)c * n + i] : mean_of(i, c);
            const double e = (y[c] - mu) / sd[c];
            q = q + e * e;
          }
          return cssm_back_lb(q);
        };
        double mx = -cssm_inf();
        for (uint32_t i = i0; i < i1; ++i) { const double lb = lb_of(i); mx = (lb > mx) ? lb : mx; }
        const double level = cssm_order_unkey(wave_max_u64(cssm_order_key(mx)));
        if (level > -cssm_inf()) {                              // (uniform)
          cssm_u128 sa = cssm_u128_zero();
          for (uint32_t i = i0; i < i1; ++i) sa = cssm_u128_add(sa, cssm_fix_from_unit(cssm_back_weight(lb_of(i), level)));
          const cssm_u128 inc = wave_scan_u128(sa, (int)lane);
          cssm_u128 tot;
          tot.lo = readlane_u64(inc.lo, 63); tot.hi = readlane_u64(inc.hi, 63);
          const double totd = cssm_u128_to_double(tot);
          const double u = cssm_back_uniform(seed, m, s);
          // C is non-decreasing: the first lane whose last slot reaches u holds the crossing (lane 63 ends at C = 1 > u)
          const unsigned long long reach = __ballot(cssm_u128_to_double(inc) / totd >= u);
          const uint32_t L = (uint32_t)__builtin_amdgcn_readfirstlane(reach ? (int)__builtin_ctzll(reach) : 63);
          const cssm_u128 exc = fleet_u128_sub(inc, sa);
          cssm_u128 before;                                     // the exact sum of the slots before lane L's
          before.lo = readlane_u64(exc.lo, (int)L); before.hi = readlane_u64(exc.hi, (int)L);
          const uint32_t f0 = (L * it < n) ? L * it : n - 1u;   // lane L's slots, one per lane
          const uint32_t f1 = (f0 + it < n) ? f0 + it : n;
          const uint32_t i = f0 + lane;
          const bool mine = i < f1;
          cssm_u128 F = cssm_fix_from_unit(cssm_back_weight(lb_of(mine ? i : f0), level));
          if (!mine) F = cssm_u128_zero();
          const cssm_u128 S = cssm_u128_add(before, wave_scan_u128(F, (int)lane));
          const unsigned long long hit = __ballot(mine && cssm_u128_to_double(S) / totd >= u);
          is = hit ? f0 + (uint32_t)__builtin_ctzll(hit) : f1 - 1u;
        }
      }
      const uint32_t js = res ? A[is] : is;
      if (lane == 0u) { s_j[t] = js; a.traj[(base + s) * M + m] = js; }
    }
  }
}

// The slices of a series, newest first, through the particles its trajectories name: fleet_lineage_body's direct source.
template <int D>
struct FleetSmoothSrc {
  static constexpr bool kDirect = true;
  const FleetSmRowArgs& a;
  size_t base; uint32_t T;
  __device__ __forceinline__ uint32_t ld() const { return a.n; }
  __device__ __forceinline__ bool resampled(uint32_t) const { return false; }
  __device__ __forceinline__ const uint32_t* anc(uint32_t j) const { return a.traj + (base + (T - j)) * a.n_traj; }
  __device__ __forceinline__ const double* cloud(uint32_t j) const { return a.hist + (base + (T - j)) * D * a.n; }
  __device__ __forceinline__ const double* fco(uint32_t j) const { return a.fco + (base + (T - j)) * D; }
  __device__ __forceinline__ double* out(uint32_t j) const { return a.out + (base + (T - j)) * (D + 1) * 3u; }
};

template <int D>
__global__ __launch_bounds__(CSSM_BLOCK) void k_fleet_smooth_rows(const FleetSmRowArgs a) {
  extern __shared__ unsigned long long s_keys[];
  __shared__ double s_p[CSSM_BLOCK / 64];
  const uint32_t k = blockIdx.x, row = blockIdx.y, tid = threadIdx.x;
  const unsigned long long r0 = a.off[k], r1 = a.off[k + 1];
  const uint32_t T = (uint32_t)(r1 - r0);
  const size_t base = (size_t)r0 + k;
  if (T == 0u || a.ser[k].err != 0u) {                          // (uniform) no records, or unusable weights: every row reads NaN
    for (uint32_t o = 0; o <= T; ++o)
      if (tid < 3u) a.out[((base + o) * (D + 1) + row) * 3u + tid] = cssm_nan();
    return;
  }
  fleet_lineage_body<D>(FleetSmoothSrc<D>{a, base, T}, T + 1u, a.n_traj, a.np2, row, a.mk, a.lo_state, a.hi_state, a.lo_eta, a.hi_eta, s_keys,
                        nullptr, s_p);
}

// (the launches go through a function template per kernel: DISPATCH_D picks the latent dimension, the template names the instantiation)
template <int D, bool STAGE>
static int backsim_launch_d(const FleetBackLaunch& l, size_t lds) {
  const uint32_t groups = (l.args.n_traj + CSSM_BACKSIM_TPB - 1u) / CSSM_BACKSIM_TPB;
  if (lds > 48u * 1024u) {                                      // beyond the default limit of a block's dynamic LDS: asked for by name
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_fleet_backsim<D, STAGE>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return (int)e;
  }
  hipLaunchKernelGGL((k_fleet_backsim<D, STAGE>), dim3(l.n_series, groups), dim3(CSSM_BLOCK), lds, l.stream, l.args);
  return (int)hipGetLastError();
}
template <int D>
static int smooth_rows_launch_d(const FleetSmRowLaunch& l) {
  hipLaunchKernelGGL(k_fleet_smooth_rows<D>, dim3(l.n_series, D + 1), dim3(CSSM_BLOCK), (size_t)l.args.np2 * 8u, l.stream, l.args);
  return (int)hipGetLastError();
}

int cssm_fleet_backsim_launch(const FleetBackLaunch& l) {
  int rc = 0;
  if (l.stage) { DISPATCH_D(l.d, rc = (backsim_launch_d<D, true>(l, (size_t)l.d * l.args.n * 8u))); }
  else { DISPATCH_D(l.d, rc = (backsim_launch_d<D, false>(l, 0))); }
  return rc;
}

int cssm_fleet_smooth_rows_launch(const FleetSmRowLaunch& l) {
  int rc = 0;
  DISPATCH_D(l.d, rc = smooth_rows_launch_d<D>(l));
  return rc;
}
