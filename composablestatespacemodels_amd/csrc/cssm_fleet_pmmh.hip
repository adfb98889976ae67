// cssm_fleet_pmmh.hip -- k_fleet_pmmh, the kernel of cssm_fleet_pmmh_chains (include/cssm_pf.h): ParticleMetropolisHastings
// (model/PMMH.scala:68-81) with the reference's prior argument (:32,72-73) and Parameters.perturbMvn (model/Parameters.scala:111-123),
// whole chains on the device.  The arithmetic is the contract's (include/cssm_numerics.h, "PMMH chains on the device"): every statement
// here is one of its functions, an existing device function of the filter (draw_normals, propagate_one, gamma_of, logdens,
// fleet_end_slot, fleet_path_row, the DPP scans), an IEEE operation or an exact integer sum, so how particles are mapped to lanes cannot
// change a bit.
//
// One workgroup per chain (grid.x = S), as k_fleet_series: a cloud of N <= CSSM_FLEET_MAX_N particles keeps its log-weights, then its
// weights, and its ancestors in LDS; the states live in HBM as x[2][D][N], ping-ponged by record parity.  The parameters are uniform
// over the block: a few threads form the proposal, the prior and the constrained fields in LDS, and per record thread c < D forms
// component c's transition coefficients and thread 0 the density constants and the level into an LDS StepRec, from a record that does
// not depend on theta (FleetIf2Rec) -- what cssm_build_rec does on the host for cssm_fleet_filter.  From there a record's statements are
// k_fleet_series's, restated here so that its instantiations stay as they are.  The chain's state (current parameters, ll, prior,
// sampled state, counters) stays in LDS across the iterations of a launch and goes to HBM between launches.  Nothing crosses a block: no
// atomics, no flags, every loop bounded by N, T_k, n_theta or the launch's iterations.
#include <hip/hip_runtime.h>

#include "cssm_internal.h"
#include "cssm_fleet_pmmh.hip.h"
#include "cssm_sde_coef.h"

template <int D>
__global__ __launch_bounds__(CSSM_FLEET_MAX_THREADS, CSSM_FLEET_WAVES(D)) void k_fleet_pmmh(const FleetPmmhArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char s_dyn[];
  __shared__ StepRec s_rec;
  __shared__ cssm_u128 s_wS[CSSM_FLEET_MAX_THREADS / 64], s_wS2[CSSM_FLEET_MAX_THREADS / 64];
  __shared__ unsigned long long s_wmax[CSSM_FLEET_MAX_THREADS / 64];
  __shared__ uint32_t s_wm[CSSM_FLEET_MAX_THREADS / 64], s_wbad[CSSM_FLEET_MAX_THREADS / 64];
  __shared__ double s_cur[CSSM_IF2_MAX_THETA], s_prop[CSSM_IF2_MAX_THETA], s_z[CSSM_IF2_MAX_THETA];
  __shared__ double s_fld[D][5];                                // the proposal's constrained m0, sqrt(c0), mu, phi, sigma per component
  __shared__ double s_cst[D], s_pst[D];                         // the sampled state: the chain's | the proposal's
  __shared__ double s_cll, s_clp, s_plp, s_pll, s_raw, s_sd;    // cur_ll, lp_cur | lp', ll' | the proposal's stored scale and its exp
  __shared__ uint32_t s_cnt[4], s_skip, s_acc;
  const uint32_t n = a.n, nt = a.n_theta, k = blockIdx.x, tid = threadIdx.x, bs = blockDim.x;
  const uint32_t lane = tid & 63u, wid = tid >> 6, nw = bs >> 6;
  double* s_lw = reinterpret_cast<double*>(s_dyn);
  uint32_t* s_anc = reinterpret_cast<uint32_t*>(s_dyn + (size_t)((n + 1u) & ~1u) * 8u);
  const unsigned long long r0 = a.off[k], r1 = a.off[k + 1];
  if (r0 >= r1) return;                                        // (uniform) no records: untouched
  const double* tab = stage_log_table(a.logtab);
  const uint32_t T = (uint32_t)(r1 - r0);
  const uint64_t seed = a.seeds[k];
  double* xb = a.x + (size_t)k * 2u * D * n;
  double* crow = a.chain + (size_t)k * CSSM_FLEET_PMMH_ROW(nt, D);
  const double* L = a.chol + (size_t)k * a.chol_stride;
  const int kind_obs = a.mk.obs_kind;
  const bool scaled = kind_obs == CSSM_OBS_GAUSSIAN || kind_obs == CSSM_OBS_NEGBIN || kind_obs == CSSM_OBS_ZIP || kind_obs == CSSM_OBS_STUDENT_T;
  const bool pow2 = (n & (n - 1u)) == 0u;
  const double inv_n = 1.0 / (double)n;
  const uint32_t it = (n + bs - 1u) / bs;                      // particles per thread of the scan phases (contiguous)
  const uint32_t j0 = tid * it;
  const uint32_t j1 = (j0 + it < n) ? j0 + it : n;             // (j0 >= n: an empty range)
  constexpr uint32_t RB = (uint32_t)CSSM_FLEET_IF2_REC_BYTES(D);
  // the chain as the launch before (or the host) left it
  for (uint32_t j = tid; j < nt; j += bs) s_cur[j] = crow[2u + j];
  if (tid < (uint32_t)D) s_cst[tid] = crow[2u + nt + tid];
  if (tid < 4u) s_cnt[tid] = a.count[(size_t)k * 4u + tid];
  if (tid == 0) { s_cll = crow[0]; s_clp = crow[1]; }
  for (uint32_t m = a.it0; m < a.it1; ++m) {                    // bounded by the launch's iterations
    const uint32_t iter = a.first_iter + m;
    const uint64_t key = cssm_derive_key(seed, (uint64_t)iter + 1u);
    __syncthreads();                                            // the chain's state stands; the iteration before is done with s_z, s_prop
    for (uint32_t j = tid; j < nt; j += bs) {
      double z0, z1;
      cssm_normal_pair_of(seed, (uint64_t)iter, j >> 1, CSSM_STREAM_HOST, 0, tab, &z0, &z1);
      s_z[j] = (j & 1u) ? z1 : z0;
    }
    __syncthreads();
    for (uint32_t i = tid; i < nt; i += bs) s_prop[i] = cssm_chain_propose(L + (size_t)i * nt, s_z, i, s_cur[i]);
    __syncthreads();
    if (tid == 0) {                                             // the prior of the proposal, its scale
      double lp = 0.0;
      for (uint32_t j = 0; j < nt; ++j) {
        const cssm_prior pr = a.priors[j];
        if (pr.kind != CSSM_PRIOR_FLAT) lp = lp + cssm_prior_term(pr.kind, pr.a, pr.b, s_prop[j]);
      }
      s_plp = lp;
      s_skip = (lp > -cssm_inf()) ? 0u : 1u;
      const double raw = (scaled && a.map.scale_slot >= 0) ? s_prop[a.map.scale_slot] : 0.0;
      s_raw = raw;
      s_sd = (scaled && a.map.scale_slot >= 0) ? cssm_exp(raw) : 1.0;
    }
    if (tid < (uint32_t)D) {                                    // component tid's constrained fields (0.0 where its SDE has none)
      const int kind = a.mk.kind((int)tid);
      double v[5];
#pragma unroll
      for (int fld = 0; fld < 5; ++fld) {
        const int slot = a.map.slot[tid][fld];
        v[fld] = slot < 0 ? 0.0 : cssm_constrain(kind, fld, s_prop[slot]);
      }
      s_fld[tid][0] = v[CSSM_FIELD_M0]; s_fld[tid][1] = cssm_sqrt(v[CSSM_FIELD_C0]);
      s_fld[tid][2] = v[CSSM_FIELD_MU]; s_fld[tid][3] = v[CSSM_FIELD_PHI]; s_fld[tid][4] = v[CSSM_FIELD_SIGMA];
    }
    __syncthreads();
    const bool skip = s_skip != 0u;                             // (uniform) outside the prior's support: rejected without a filter
    uint32_t err = 0u;
    double ll = 0.0;
    if (!skip) {
      // initialiseState: x0 = sqrt(c0) z + m0 into buffer 0, identity ancestors
      for (uint32_t i = tid; i < n; i += bs) {
        double z[D];
        draw_normals<D>(key, (uint64_t)i, 0u, CSSM_STREAM_INIT, tab, z);
#pragma unroll
        for (int c = 0; c < D; ++c) xb[(size_t)c * n + i] = s_fld[c][1] * z[c] + s_fld[c][0];
        s_anc[i] = i;
      }
      for (unsigned long long r = r0; r < r1; ++r) {            // bounded by the series' length
        __syncthreads();                                        // the cloud / ancestors of the record before; s_rec is free
        {
          const unsigned char* g = a.recs + (size_t)r * RB;
          const FleetIf2Rec* h = reinterpret_cast<const FleetIf2Rec*>(g);
          const double* tail = reinterpret_cast<const double*>(g + sizeof(FleetIf2Rec));
          if (tid == 0) {                                       // cssm_build_rec's scalars under the proposal
            double cc[4] = {0.0, 0.0, 0.0, 0.0}, cdf = 0.0;
            if (h->has_obs) cssm_obs_consts(kind_obs, h->y, h->ypart, s_sd, s_raw, a.df, cc, &cdf);
            s_rec.y = cssm_obs_y(kind_obs, h->y);
            s_rec.c[0] = cc[0]; s_rec.c[1] = cc[1]; s_rec.c[2] = cc[2]; s_rec.c[3] = cc[3]; s_rec.cdf = cdf;
            s_rec.u = cssm_if2_uniform(key, h->step);
            s_rec.dt = h->dt;
            s_rec.ref = h->has_obs ? cssm_ref_level(kind_obs, h->y, s_sd, a.df) : cssm_nan();
            s_rec.has_obs = h->has_obs; s_rec.step = h->step;
          }
          if (tid < (uint32_t)D) {
            cssm_sde_coef(a.mk.kind((int)tid), s_fld[tid][2], s_fld[tid][3], s_fld[tid][4], h->dt, s_rec.coef[tid]);
            s_rec.fco[tid] = tail[tid];
          }
        }
        __syncthreads();
        const StepRec* rec = &s_rec;
        const uint32_t step = rec->step;
        const bool weighted = rec->has_obs != 0;
        const double* src = xb + (size_t)(step & 1u) * D * n;
        double* dst = xb + (size_t)((step & 1u) ^ 1u) * D * n;
        // 1. gather through the previous ancestors, transition, f, log-density
        double tmax = -cssm_inf();
        bool bad = false;
        for (uint32_t i = tid; i < n; i += bs) {
          const uint32_t j = s_anc[i];
          double x[D];
#pragma unroll
          for (int c = 0; c < D; ++c) x[c] = src[(size_t)c * n + j];
          propagate_one<D>(a.mk, rec, rec->dt, key, (uint64_t)i, step, tab, x);
#pragma unroll
          for (int c = 0; c < D; ++c) dst[(size_t)c * n + i] = x[c];
          if (weighted) {
            double lw = logdens<-1>(a.mk, rec, gamma_of<D>(a.mk, rec, x), tab);
            if (lw != lw) { bad = true; lw = -cssm_inf(); }
            tmax = (lw > tmax) ? lw : tmax;
            s_lw[i] = lw;
          }
        }
        if (!weighted) {                                        // (uniform) the None branch: the cloud moves, nothing else
          __syncthreads();
          for (uint32_t i = tid; i < n; i += bs) s_anc[i] = i;
          continue;
        }
        // 2. the block's own max: the level is chosen in place
        {
          const unsigned long long km = wave_max_u64(cssm_order_key(tmax));
          const bool anyb = __any(bad);
          if (lane == 0u) { s_wmax[wid] = km; s_wbad[wid] = anyb ? 1u : 0u; }
        }
        __syncthreads();
        unsigned long long kmax = 0ull; uint32_t anybad = 0u;
        for (uint32_t w = 0; w < nw; ++w) { kmax = (s_wmax[w] > kmax) ? s_wmax[w] : kmax; anybad |= s_wbad[w]; }
        const double gmax = cssm_order_unkey(kmax);
        if (anybad || !(gmax > -cssm_inf()) || !(gmax < cssm_inf())) { err = anybad ? 1u : 2u; break; }   // (uniform) no usable weight
        const double ref = cssm_ref_choose(rec->ref, gmax);
        // 3. weights on the 2^-96 grid, their sums, the block scan
        cssm_u128 sa = cssm_u128_zero(), sb = cssm_u128_zero();
        for (uint32_t j = j0; j < j1; ++j) {
          const double w1 = cssm_exp_le0(cssm_min_c(s_lw[j] - ref, CSSM_REF_BELOW));
          s_lw[j] = w1;
          sa = cssm_u128_add(sa, cssm_fix_from_unit(w1));
          sb = cssm_u128_add(sb, cssm_fix_from_unit(w1 * w1));
        }
        for (uint32_t i = tid; i < n; i += bs) s_anc[i] = 0u;  // (every thread gathered before the barrier above)
        const cssm_u128 inc = wave_scan_u128(sa, (int)lane);
        const cssm_u128 wb2 = wave_sum_u128(sb);
        if (lane == 63u) { s_wS[wid] = inc; s_wS2[wid] = wb2; }
        __syncthreads();
        cssm_u128 tot = cssm_u128_zero(), tot2 = cssm_u128_zero(), off = cssm_u128_zero();
        for (uint32_t w = 0; w < nw; ++w) {
          if (w < wid) off = cssm_u128_add(off, s_wS[w]);
          tot = cssm_u128_add(tot, s_wS[w]); tot2 = cssm_u128_add(tot2, s_wS2[w]);
        }
        if (cssm_u128_is_zero(tot)) { err = 2u; break; }        // (uniform)
        ll = ll + ref + cssm_log(cssm_fix_to_double(tot) / (double)n);
        // 4. systematic resampling: particle j drops its index at the first slot of its run, an inclusive max-scan fills the runs
        {
          const double totd = cssm_u128_to_double(tot);
          const double u = rec->u;
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
      }
      __syncthreads();
      if (!err) {                                               // (uniform) row T of the sampled path: record T - 1 wrote buffer T & 1
        const int32_t pr = (int32_t)cssm_philox_draw(key, 0, T, CSSM_STREAM_PICK, 0).v[0];
        const uint32_t pick = (uint32_t)((uint64_t)(pr < 0 ? (uint32_t)0 - (uint32_t)pr : (uint32_t)pr) % n);
        fleet_path_row<D>(xb + (size_t)(T & 1u) * D * n, s_anc, n, pick, s_pst, tid);
      }
    }
    // the decision (PMMH.scala:72-75)
    if (tid == 0) {
      const cssm_u32x4 b = cssm_philox_draw(seed, (uint64_t)iter, 0xffffffffu, CSSM_STREAM_HOST, 1);
      const double uu = cssm_u01_open0(b.v[0], b.v[1]);
      const double pll = err ? -cssm_inf() : ll;
      bool acc = false;
      if (!skip) acc = cssm_log(uu) < cssm_chain_log_ratio(pll, s_plp, s_cll, s_clp);
      s_pll = pll;
      s_acc = acc ? 1u : 0u;
      s_cnt[0] += acc ? 1u : 0u; s_cnt[1] += skip ? 1u : 0u; s_cnt[2] += (!skip && err) ? 1u : 0u;
    }
    __syncthreads();
    if (s_acc) {                                                // (uniform)
      for (uint32_t j = tid; j < nt; j += bs) s_cur[j] = s_prop[j];
      if (tid < (uint32_t)D) s_cst[tid] = s_pst[tid];
      if (tid == 0) { s_cll = s_pll; s_clp = s_plp; }
      __syncthreads();
    }
    {                                                           // the iteration's row
      const size_t row = (size_t)k * a.n_iters + m;
      for (uint32_t j = tid; j < nt; j += bs) a.theta[row * nt + j] = s_cur[j];
      if (tid < (uint32_t)D) a.last[row * D + tid] = s_cst[tid];
      if (tid == 0) { a.ll[row] = s_cll; a.accepted[row] = (int32_t)s_cnt[0]; }
    }
  }
  __syncthreads();
  for (uint32_t j = tid; j < nt; j += bs) crow[2u + j] = s_cur[j];
  if (tid < (uint32_t)D) crow[2u + nt + tid] = s_cst[tid];
  if (tid < 4u) a.count[(size_t)k * 4u + tid] = s_cnt[tid];
  if (tid == 0) { crow[0] = s_cll; crow[1] = s_clp; }
}

template <int D>
static int pmmh_launch_d(const FleetPmmhLaunch& l) {
  hipLaunchKernelGGL(k_fleet_pmmh<D>, dim3(l.n_series), dim3(l.threads), l.lds, l.stream, l.args);
  return (int)hipGetLastError();
}

int cssm_fleet_pmmh_launch(const FleetPmmhLaunch& l) {
  int rc = 0;
  DISPATCH_D(l.d, rc = pmmh_launch_d<D>(l));
  return rc;
}
