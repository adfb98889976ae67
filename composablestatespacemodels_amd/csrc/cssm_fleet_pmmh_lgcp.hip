// cssm_fleet_pmmh_lgcp.hip -- k_fleet_pmmh_lgcp, the kernel of cssm_fleet_pmmh_chains_lgcp (include/cssm_pf.h): ParticleMetropolisHastings
// (model/PMMH.scala:68-81) over FilterLgcp (model/ParticleFilter.scala:169-227), whole chains on the device.  The arithmetic is the
// contract's (include/cssm_numerics.h, "PMMH chains on the device: LGCP"): the iteration around the filter is k_fleet_pmmh's statement for
// statement (cssm_fleet_pmmh.hip), the filter inside it is k_fleet_series<D, PATH, ..., LGCP = true>'s (cssm_fleet.hip.h) with the sub-step
// walk it calls (fleet_lgcp_weigh, cssm_fleet_lgcp.hip.h), both restated here so that their instantiations stay as they are.
//
// One workgroup per chain (grid.x = S): the cloud's log-weights, then its weights, and its ancestors in LDS, the states in HBM as
// x[2][D][N] ping-ponged by event parity.  Every sub-step of every event has the increment delta, so thread c < D forms component c's four
// transition coefficients ONCE PER ITERATION -- cssm_sde_coef over delta, the bits cssm_build_rec writes into an LGCP StepRec -- and an
// event only brings what does not depend on theta (FleetPmmhLgcpRec): n_sub, the observation index, F at its time and where its rows of
// the sub-step table start.  The predicted level (contract v8) is a register that starts as NaN with every iteration's filter.  Nothing
// crosses a block: no atomics, no flags, every loop bounded by N, T_k, n_sub, n_theta or the launch's iterations.
#include <hip/hip_runtime.h>

#include "cssm_internal.h"
#include "cssm_fleet_pmmh_lgcp.hip.h"
#include "cssm_sde_coef.h"

template <int D>
__global__ __launch_bounds__(CSSM_FLEET_MAX_THREADS, CSSM_FLEET_WAVES(D)) void k_fleet_pmmh_lgcp(const FleetPmmhLgcpArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char s_dyn[];
  __shared__ StepRec s_rec;
  __shared__ cssm_u128 s_wS[CSSM_FLEET_MAX_THREADS / 64], s_wS2[CSSM_FLEET_MAX_THREADS / 64];
  __shared__ unsigned long long s_wmax[CSSM_FLEET_MAX_THREADS / 64];
  __shared__ uint32_t s_wm[CSSM_FLEET_MAX_THREADS / 64], s_wbad[CSSM_FLEET_MAX_THREADS / 64];
  __shared__ double s_cur[CSSM_IF2_MAX_THETA], s_prop[CSSM_IF2_MAX_THETA], s_z[CSSM_IF2_MAX_THETA];
  __shared__ double s_ini[D][2];                                // the proposal's constrained m0, sqrt(c0) per component
  __shared__ double s_cst[D], s_pst[D];                         // the sampled state: the chain's | the proposal's
  __shared__ double s_cll, s_clp, s_plp, s_pll;                 // cur_ll, lp_cur | lp', ll'
  __shared__ uint32_t s_cnt[4], s_skip, s_acc;
  const uint32_t n = a.n, nt = a.n_theta, k = blockIdx.x, tid = threadIdx.x, bs = blockDim.x;
  const uint32_t lane = tid & 63u, wid = tid >> 6, nw = bs >> 6;
  double* s_lw = reinterpret_cast<double*>(s_dyn);
  uint32_t* s_anc = reinterpret_cast<uint32_t*>(s_dyn + (size_t)((n + 1u) & ~1u) * 8u);
  const unsigned long long r0 = a.off[k], r1 = a.off[k + 1];
  if (r0 >= r1) return;                                        // (uniform) no events: untouched
  const double* tab = stage_log_table(a.logtab);
  const uint32_t T = (uint32_t)(r1 - r0);
  const uint64_t seed = a.seeds[k];
  double* xb = a.x + (size_t)k * 2u * D * n;
  double* crow = a.chain + (size_t)k * CSSM_FLEET_PMMH_ROW(nt, D);
  const double* L = a.chol + (size_t)k * a.chol_stride;
  const bool pow2 = (n & (n - 1u)) == 0u;
  const double inv_n = 1.0 / (double)n;
  const uint32_t it = (n + bs - 1u) / bs;                      // particles per thread of the scan phases (contiguous)
  const uint32_t j0 = tid * it;
  const uint32_t j1 = (j0 + it < n) ? j0 + it : n;             // (j0 >= n: an empty range)
  constexpr uint32_t RB = (uint32_t)CSSM_FLEET_PMMH_LGCP_REC_BYTES(D);
  // the chain as the launch before (or the host) left it
  for (uint32_t j = tid; j < nt; j += bs) s_cur[j] = crow[2u + j];
  if (tid < (uint32_t)D) s_cst[tid] = crow[2u + nt + tid];
  if (tid < 4u) s_cnt[tid] = a.count[(size_t)k * 4u + tid];
  if (tid == 0) { s_cll = crow[0]; s_clp = crow[1]; }
  for (uint32_t m = a.it0; m < a.it1; ++m) {                    // bounded by the launch's iterations
    const uint32_t iter = a.first_iter + m;
    const uint64_t key = cssm_derive_key(seed, (uint64_t)iter + 1u);
    __syncthreads();                                            // the chain's state stands; the iteration before is done with s_z, s_prop, s_rec
    for (uint32_t j = tid; j < nt; j += bs) {
      double z0, z1;
      cssm_normal_pair_of(seed, (uint64_t)iter, j >> 1, CSSM_STREAM_HOST, 0, tab, &z0, &z1);
      s_z[j] = (j & 1u) ? z1 : z0;
    }
    __syncthreads();
    for (uint32_t i = tid; i < nt; i += bs) s_prop[i] = cssm_chain_propose(L + (size_t)i * nt, s_z, i, s_cur[i]);
    __syncthreads();
    if (tid == 0) {                                             // the prior of the proposal
      double lp = 0.0;
      for (uint32_t j = 0; j < nt; ++j) {
        const cssm_prior pr = a.priors[j];
        if (pr.kind != CSSM_PRIOR_FLAT) lp = lp + cssm_prior_term(pr.kind, pr.a, pr.b, s_prop[j]);
      }
      s_plp = lp;
      s_skip = (lp > -cssm_inf()) ? 0u : 1u;
    }
    if (tid < (uint32_t)D) {                                    // component tid's constrained fields (0.0 where its SDE has none) ...
      const int kind = a.mk.kind((int)tid);
      double v[5];
#pragma unroll
      for (int fld = 0; fld < 5; ++fld) {
        const int slot = a.map.slot[tid][fld];
        v[fld] = slot < 0 ? 0.0 : cssm_constrain(kind, fld, s_prop[slot]);
      }
      s_ini[tid][0] = v[CSSM_FIELD_M0]; s_ini[tid][1] = cssm_sqrt(v[CSSM_FIELD_C0]);
      // ... and its transition coefficients over delta: every sub-step of every event of this iteration reads them
      cssm_sde_coef(kind, v[CSSM_FIELD_MU], v[CSSM_FIELD_PHI], v[CSSM_FIELD_SIGMA], a.delta, s_rec.coef[tid]);
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
        for (int c = 0; c < D; ++c) xb[(size_t)c * n + i] = s_ini[c][1] * z[c] + s_ini[c][0];
        s_anc[i] = i;
      }
      double next_ref = cssm_nan();                             // no event of this filter yet whose max could predict a level
      for (unsigned long long r = r0; r < r1; ++r) {            // bounded by the series' length
        __syncthreads();                                        // the cloud / ancestors of the event before; s_rec's event fields are free
        {
          const unsigned char* g = a.recs + (size_t)r * RB;
          const FleetPmmhLgcpRec* h = reinterpret_cast<const FleetPmmhLgcpRec*>(g);
          const double* tail = reinterpret_cast<const double*>(g + sizeof(FleetPmmhLgcpRec));
          if (tid == 0) {
            s_rec.u = cssm_if2_uniform(key, h->step);
            s_rec.dt = h->dt; s_rec.n_sub = h->n_sub; s_rec.step = h->step; s_rec.fsub_off = h->fsub_off; s_rec.has_obs = 1;
          }
          if (tid < (uint32_t)D) s_rec.fco[tid] = tail[tid];
        }
        __syncthreads();
        const StepRec* rec = &s_rec;
        const uint32_t step = rec->step;
        const double* src = xb + (size_t)(step & 1u) * D * n;
        double* dst = xb + (size_t)((step & 1u) ^ 1u) * D * n;
        // 1. gather through the previous ancestors, the event's sub-steps, gamma - hazard.  W of the thread's particles at a time; a lane
        //    whose group is short walks its first particle again and stores nothing of it
        double tmax = -cssm_inf();
        bool bad = false;
        constexpr int W = CSSM_FLEET_LGCP_WIDTH;
        for (uint32_t i0 = tid; i0 < n; i0 += (uint32_t)W * bs) {
          double x[W][D], lw[W];
          uint32_t gid[W];
#pragma unroll
          for (int q = 0; q < W; ++q) {
            const uint32_t i = i0 + (uint32_t)q * bs;
            gid[q] = (i < n) ? i : i0;
            const uint32_t j = s_anc[gid[q]];
#pragma unroll
            for (int c = 0; c < D; ++c) x[q][c] = src[(size_t)c * n + j];
          }
          fleet_lgcp_weigh<D, W>(a.mk, rec, a.fsub, key, gid, tab, x, lw);
#pragma unroll
          for (int q = 0; q < W; ++q) {
            const uint32_t i = i0 + (uint32_t)q * bs;
            if (i < n) {
#pragma unroll
              for (int c = 0; c < D; ++c) dst[(size_t)c * n + i] = x[q][c];
              double w = lw[q];
              if (w != w) { bad = true; w = -cssm_inf(); }
              tmax = (w > tmax) ? w : tmax;
              s_lw[i] = w;
            }
          }
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
        const double ref = cssm_ref_choose(next_ref, gmax);     // the level predicted from the event before; this event's max predicts the next
        next_ref = cssm_ref_predict(gmax);
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
      if (!err) {                                               // (uniform) row T of the sampled path: event T - 1 wrote buffer T & 1
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
static int pmmh_lgcp_launch_d(const FleetPmmhLgcpLaunch& l) {
  hipLaunchKernelGGL(k_fleet_pmmh_lgcp<D>, dim3(l.n_series), dim3(l.threads), l.lds, l.stream, l.args);
  return (int)hipGetLastError();
}

int cssm_fleet_pmmh_lgcp_launch(const FleetPmmhLgcpLaunch& l) {
  int rc = 0;
  DISPATCH_D(l.d, rc = pmmh_lgcp_launch_d<D>(l));
  return rc;
}
