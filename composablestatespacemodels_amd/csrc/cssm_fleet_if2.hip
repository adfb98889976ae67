// cssm_fleet_if2.hip -- k_fleet_if2, the kernel of cssm_fleet_if2 (include/cssm_pf.h).  EXTENSION: iterated filtering (IF2; Ionides,
// Nguyen, Atchade, Stoev and King 2015); the reference has no likelihood maximiser.  The arithmetic is the contract's
// (include/cssm_numerics.h, "iterated filtering"): every statement here is one of its functions, an existing device function of the
// filter (draw_normals, cssm_sde_coef, transition_step, gamma_coef, fleet_end_slot, the DPP scans), an IEEE operation or an exact integer
// sum, so how particles are mapped to lanes cannot change a bit.
//
// One workgroup per series (grid.x = S), as k_fleet_series: a cloud of N <= CSSM_FLEET_MAX_N particles keeps its log-weights, then its
// weights, and its ancestors in LDS.  New is that every particle carries its own parameter vector: the swarm lives in HBM as
// theta[2][n_theta][N] next to x[2][D][N], both ping-ponged by record parity and read through the ancestors, the parameters streamed
// slot by slot (a row has up to 81 of them).  The loop over iterations and records runs inside the kernel: transition coefficients and
// density constants are formed per particle, so a record does not depend on theta and the host has nothing to do between iterations.
// Steps 2-4 of a record (level, fixed-point sums, systematic resampling) are k_fleet_series's statements, restated here so that its
// instantiations stay as they are.  Nothing crosses a block: no atomics, no flags, every loop bounded by N, T_k, n_theta or the launch's
// iterations.
#include <hip/hip_runtime.h>

#include "cssm_internal.h"
#include "cssm_fleet_if2.hip.h"
#include "cssm_if2_move.hip.h"
#include "cssm_sde_coef.h"

template <int D>
__global__ __launch_bounds__(CSSM_FLEET_MAX_THREADS, CSSM_FLEET_WAVES(D)) void k_fleet_if2(const FleetIf2Args a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char s_dyn[];
  __shared__ FleetIf2Rec s_rec;
  __shared__ double s_fco[D], s_u;
  __shared__ double s_sd0[CSSM_IF2_MAX_THETA + 3], s_sdr[CSSM_IF2_MAX_THETA + 3];   // sd_j cool_m: before x0 | before a record (0 for m0, c0)
  __shared__ cssm_u128 s_wS[CSSM_FLEET_MAX_THREADS / 64], s_wS2[CSSM_FLEET_MAX_THREADS / 64];
  __shared__ unsigned long long s_wmax[CSSM_FLEET_MAX_THREADS / 64], s_wref[CSSM_FLEET_MAX_THREADS / 64];
  __shared__ uint32_t s_wm[CSSM_FLEET_MAX_THREADS / 64];
  const uint32_t n = a.n, nt = a.n_theta, k = blockIdx.x, tid = threadIdx.x, bs = blockDim.x;
  const uint32_t lane = tid & 63u, wid = tid >> 6, nw = bs >> 6;
  double* s_lw = reinterpret_cast<double*>(s_dyn);
  uint32_t* s_anc = reinterpret_cast<uint32_t*>(s_dyn + (size_t)((n + 1u) & ~1u) * 8u);
  const unsigned long long r0 = a.off[k], r1 = a.off[k + 1];
  if (r0 >= r1) return;                                        // (uniform) no records: untouched
  if (a.ser[k].err != 0u) return;                              // (uniform) the search ended in an earlier launch
  const double* tab = stage_log_table(a.logtab);
  const uint32_t T = (uint32_t)(r1 - r0);
  const uint64_t seed = a.seeds[k];
  double* sw = a.swarm + (size_t)k * nt * n;
  double* thb = a.theta + (size_t)k * 2u * nt * n;
  double* xb = a.x + (size_t)k * 2u * D * n;
  const int kind_obs = a.mk.obs_kind;
  const bool scaled = kind_obs == CSSM_OBS_GAUSSIAN || kind_obs == CSSM_OBS_NEGBIN || kind_obs == CSSM_OBS_ZIP || kind_obs == CSSM_OBS_STUDENT_T;
  const bool own_level = kind_obs == CSSM_OBS_GAUSSIAN || kind_obs == CSSM_OBS_STUDENT_T;   // cssm_ref_level depends on the particle's scale
  const bool pow2 = (n & (n - 1u)) == 0u;
  const double inv_n = 1.0 / (double)n;
  const uint32_t it = (n + bs - 1u) / bs;                      // particles per thread of the scan phases (contiguous)
  const uint32_t j0 = tid * it;
  const uint32_t j1 = (j0 + it < n) ? j0 + it : n;
  constexpr uint32_t RB = (uint32_t)CSSM_FLEET_IF2_REC_BYTES(D);
  uint32_t err = 0u;
  for (uint32_t m = a.it0; m < a.it1 && !err; ++m) {            // bounded by the launch's iterations
    const uint64_t key = cssm_derive_key(seed, (uint64_t)a.first_iter + m + 1u);
    __syncthreads();                                            // the iteration before is done with s_sd*, s_lw, theta
    for (uint32_t j = tid; j < CSSM_IF2_MAX_THETA + 3u; j += bs) {
      const double sdc = (j < nt) ? a.rw_sd[j] * a.cool[m] : 0.0;
      s_sd0[j] = sdc;
      s_sdr[j] = (j < nt && a.map.ivp[j]) ? 0.0 : sdc;
    }
    __syncthreads();
    // the swarm, perturbed (every slot: pomp's ivp slots here and only here), into buffer 0; x0 from the particle's own m0, c0
    for (uint32_t i = tid; i < n; i += bs) {
      if2_move(sw, i, thb, i, n, nt, key, 0u, s_sd0, tab);
      double z[D];
      draw_normals<D>(key, (uint64_t)i, 0u, CSSM_STREAM_INIT, tab, z);
#pragma unroll
      for (int c = 0; c < D; ++c) {
        const int kind = a.mk.kind(c);
        const double m0 = if2_field(a.map, kind, c, CSSM_FIELD_M0, thb, i, n), c0 = if2_field(a.map, kind, c, CSSM_FIELD_C0, thb, i, n);
        xb[(size_t)c * n + i] = cssm_sqrt(c0) * z[c] + m0;
      }
      s_anc[i] = i;
    }
    double ll = 0.0; int32_t ess = (int32_t)n;
    for (unsigned long long r = r0; r < r1; ++r) {              // bounded by the series' length
      __syncthreads();                                          // the cloud / swarm / ancestors of the record before; s_rec is free
      {
        const unsigned char* g = a.recs + (size_t)r * RB;
        const FleetIf2Rec* h = reinterpret_cast<const FleetIf2Rec*>(g);
        const double* tail = reinterpret_cast<const double*>(g + sizeof(FleetIf2Rec));
        if (tid == 0) { s_rec = *h; s_u = cssm_if2_uniform(key, h->step); }
        if (tid < (uint32_t)D) s_fco[tid] = tail[tid];
      }
      __syncthreads();
      const uint32_t step = s_rec.step;
      const bool weighted = s_rec.has_obs != 0;
      const double dt = s_rec.dt, y = s_rec.y, ypart = s_rec.ypart;
      const double yk = cssm_obs_y(kind_obs, y);
      const double* tsrc = thb + (size_t)(step & 1u) * nt * n;
      double* tdst = thb + (size_t)((step & 1u) ^ 1u) * nt * n;
      const double* xsrc = xb + (size_t)(step & 1u) * D * n;
      double* xdst = xb + (size_t)((step & 1u) ^ 1u) * D * n;
      // 1. gather theta and x through the previous ancestors, perturb, the particle's own coefficients, transition, f, log-density
      double tmax = -cssm_inf(), cmax = -cssm_inf();
      for (uint32_t i = tid; i < n; i += bs) {
        const uint32_t j = s_anc[i];
        if2_move(tsrc, j, tdst, i, n, nt, key, step + 1u, s_sdr, tab);
        double x[D], z[D];
        draw_normals<D>(key, (uint64_t)i, step, CSSM_STREAM_STEP, tab, z);
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
          double lw = cssm_obs_logdens(kind_obs, yk, cc, cdf, gamma_coef<D>(a.mk, s_fco, x));
          if (lw != lw) lw = -cssm_inf();                       // a NaN log-weight is weight zero, not the end of the search
          tmax = (lw > tmax) ? lw : tmax;
          s_lw[i] = lw;
          if (own_level) { const double cl = cssm_if2_level(kind_obs, y, sd, a.df); cmax = (cl > cmax) ? cl : cmax; }
        }
      }
      if (!weighted) {                                          // (uniform) the cloud and the swarm move, nothing else
        __syncthreads();
        for (uint32_t i = tid; i < n; i += bs) s_anc[i] = i;
        if (tid == 0 && a.ll_t) a.ll_t[r] = ll;
        if (tid == 0 && a.ess_t) a.ess_t[r] = ess;
        continue;
      }
      // 2. the block's own maxima: of the log-weights, and of the particles' level candidates
      {
        const unsigned long long km = wave_max_u64(cssm_order_key(tmax));
        const unsigned long long kc = wave_max_u64(cssm_order_key(cmax));
        if (lane == 0u) { s_wmax[wid] = km; s_wref[wid] = kc; }
      }
      __syncthreads();
      unsigned long long kmax = 0ull, kcmax = 0ull;
      for (uint32_t w = 0; w < nw; ++w) { kmax = (s_wmax[w] > kmax) ? s_wmax[w] : kmax; kcmax = (s_wref[w] > kcmax) ? s_wref[w] : kcmax; }
      const double gmax = cssm_order_unkey(kmax);
      if (!(gmax > -cssm_inf()) || !(gmax < cssm_inf())) { err = 2u; break; }   // (uniform) no particle has a usable weight
      const double ref = cssm_ref_choose(own_level ? cssm_order_unkey(kcmax) : s_rec.ref, gmax);
      // 3. weights on the 2^-96 grid, their sums, the block scan
      cssm_u128 sa = cssm_u128_zero(), sb = cssm_u128_zero();
      for (uint32_t j = j0; j < j1; ++j) {
        const double w1 = cssm_exp_le0(cssm_min_c(s_lw[j] - ref, CSSM_REF_BELOW));
        s_lw[j] = w1;
        sa = cssm_u128_add(sa, cssm_fix_from_unit(w1));
        sb = cssm_u128_add(sb, cssm_fix_from_unit(w1 * w1));
      }
      for (uint32_t i = tid; i < n; i += bs) s_anc[i] = 0u;    // (every thread gathered before the barrier above)
      const cssm_u128 inc = wave_scan_u128(sa, (int)lane);
      const cssm_u128 wb2 = wave_sum_u128(sb);
      if (lane == 63u) { s_wS[wid] = inc; s_wS2[wid] = wb2; }
      __syncthreads();
      cssm_u128 tot = cssm_u128_zero(), tot2 = cssm_u128_zero(), off = cssm_u128_zero();
      for (uint32_t w = 0; w < nw; ++w) {
        if (w < wid) off = cssm_u128_add(off, s_wS[w]);
        tot = cssm_u128_add(tot, s_wS[w]); tot2 = cssm_u128_add(tot2, s_wS2[w]);
      }
      if (cssm_u128_is_zero(tot)) { err = 2u; break; }          // (uniform)
      ll = ll + ref + cssm_log(cssm_fix_to_double(tot) / (double)n);
      ess = cssm_ess_of(tot, tot2);
      // 4. systematic resampling: particle j drops its index at the first slot of its run, an inclusive max-scan fills the runs
      {
        const double totd = cssm_u128_to_double(tot);
        const double u = s_u;
        cssm_u128 run = fleet_u128_sub(cssm_u128_add(off, inc), sa);
        uint32_t prev = 0u;
        if (j0 < j1 && j0 > 0u) prev = fleet_end_slot(run, totd, u, n, pow2, inv_n);
        for (uint32_t j = j0; j < j1; ++j) {
          run = cssm_u128_add(run, cssm_fix_from_unit(s_lw[j]));
          const uint32_t e = fleet_end_slot(run, totd, u, n, pow2, inv_n);
          if (e > prev) s_anc[prev] = j;
          prev = (e > prev) ? e : prev;
        }
      }
      __syncthreads();
      {
        uint32_t mx = 0u;
        for (uint32_t s = j0; s < j1; ++s) { const uint32_t v = s_anc[s]; mx = (v > mx) ? v : mx; }
        const uint32_t incl = wave_scan_max_u32(mx);
        uint32_t carry = dpp0<0x138 /* wave_shr:1 */, 0xf>(incl);
        if (lane == 63u) s_wm[wid] = incl;
        __syncthreads();
        for (uint32_t w = 0; w < wid; ++w) carry = (s_wm[w] > carry) ? s_wm[w] : carry;
        for (uint32_t s = j0; s < j1; ++s) {
          const uint32_t v = s_anc[s];
          carry = (v > carry) ? v : carry;
          s_anc[s] = carry;
        }
      }
      if (tid == 0 && a.ll_t) a.ll_t[r] = ll;
      if (tid == 0 && a.ess_t) a.ess_t[r] = ess;
    }
    if (err) {                                                  // (uniform) the swarm stays the one this iteration started from
      if (tid == 0) { FleetIf2Series o; o.err = err; o.fail_iter = m; a.ser[k] = o; }
      break;
    }
    // the swarm of the next iteration: theta through the last ancestors; per slot its mean, a pairwise tree over the particle index
    __syncthreads();
    const double* tfin = thb + (size_t)(T & 1u) * nt * n;       // record T - 1 wrote buffer T & 1
    for (uint32_t j = 0; j < nt; ++j) {
      for (uint32_t i = tid; i < n; i += bs) {
        const double v = tfin[(size_t)j * n + s_anc[i]];
        sw[(size_t)j * n + i] = v;
        s_lw[i] = v;
      }
      for (uint32_t stride = 1u; stride < n; stride <<= 1) {    // level l pairs the elements at i 2^(l+1) and i 2^(l+1) + 2^l
        __syncthreads();
        for (uint32_t i = tid * 2u * stride; i < n; i += bs * 2u * stride)
          s_lw[i] = s_lw[i] + ((i + stride < n) ? s_lw[i + stride] : 0.0);
      }
      __syncthreads();
      if (tid == 0) a.theta_mean[((size_t)k * a.n_iters + m) * nt + j] = s_lw[0] / (double)n;
      __syncthreads();                                          // s_lw is the next slot's
    }
    if (tid == 0) a.ll[(size_t)k * a.n_iters + m] = ll;
    if (a.anc_out && m + 1u == a.it1)
      for (uint32_t i = tid; i < n; i += bs) a.anc_out[(size_t)k * n + i] = s_anc[i];
  }
}

template <int D>
static int if2_launch_d(const FleetIf2Launch& l) {
  hipLaunchKernelGGL(k_fleet_if2<D>, dim3(l.n_series), dim3(l.threads), l.lds, l.stream, l.args);
  return (int)hipGetLastError();
}

int cssm_fleet_if2_launch(const FleetIf2Launch& l) {
  int rc = 0;
  DISPATCH_D(l.d, rc = if2_launch_d<D>(l));
  return rc;
}
