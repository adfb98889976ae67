// cssm_fleet_onestep.hip.h -- the one-step-ahead forecast of ONE record by the workgroup that filters it (k_fleet_series<D, false, false,
// false, true>: cssm_fleet_filter_forecasts, cssm_fleet_step_forecast).  ParticleFilter.getMeanForecast mapped over a filter stream
// (model/ParticleFilter.scala:368-409): from the cloud BEFORE the record, the time of the record, before the record is weighed -- what
// cssm_fleet_forecast returns for the series with the single horizon t[r], issued just before the record is stepped.
//
// Every arithmetic statement is k_fleet_forecast's, in its order: a pair gathered through the ancestors, propagate_pair / propagate_one on
// the paired CSSM_STREAM_STEP streams under the record's forecast key at horizon index 0, gamma_of, link_of, cssm_obs_draw_one on
// cssm_obs_stream_at, the row summaries of cssm_fleet_intervals.hip.h (fleet_row_keys, fleet_sort_keys).  What is new is where the
// operands live: the record's own StepRec in LDS carries dt, the transition and the f coefficients of t[r]; the states go to the record's
// DESTINATION buffer, which the record's own propagate overwrites afterwards; the keys of a row's sort live where the weights were.
#pragma once

#include "cssm_device.hip.h"
#include "cssm_fleet_intervals.hip.h"
#include "../../include/cssm_obs_draws.h"

#define CSSM_FLEET_FC_ON 1u    /* FleetOneStep::flags: the record has a forecast row (its time is finite and not before the series' clock) */
#define CSSM_FLEET_FC_HAS 2u   /* ... and a datum: the PIT counts are taken against FleetOneStep::y */

// What a launch that also forecasts every record carries, per record of the launch (keys / y / flags), per series (op / stage) and per
// result row (out / pit; the row of record r is r, or -- FleetArgs::iv_rows == 1, the step form -- the series' number)
struct FleetOneStep {
  const unsigned long long* keys;    // the Philox key of the record's forecast
  const double* y;                   // the datum as the caller gave it (StepRec::y is the density's: truncated for a count)
  const uint32_t* flags;             // CSSM_FLEET_FC_*
  const cssm_obs_params* op;         // [S]: the series' observation parameters
  double* stage;                     // [S][2][n]: eta and the observation draw of the record at hand
  double* out;                       // rows of [d + 2][3] (mean, lower, upper: the d states, eta, obs), preset to NaN
  int32_t* pit;                      // rows of 2: the draws strictly below / equal to y, preset to -1
};

// Every thread of the block calls it, behind a barrier that completed the cloud in `src`, `s_anc` and *rec; it ends behind a barrier of
// its own, so `dst` and `s_keys` (np2 keys of LDS nothing else uses meanwhile) are free again on return.  s_p / s_cnt: one double / two
// counts per wave.  Every loop is bounded by n, np2, D or the block's waves.  Inlined: as a real call (__noinline__) the phase cost every
// dimension 900 - 1200 bytes of scratch per lane instead of 200 - 860.
template <int D>
__device__ __forceinline__ void fleet_onestep_forecast(const ModelK& mk, const StepRec* rec, const double* src, double* dst, const uint32_t* s_anc,
                                                       uint32_t n, uint32_t np2, uint64_t key, const cssm_obs_params op, double* stage,
                                                       const double* tab, const FleetRowRanks& rk, unsigned long long* s_keys, double* s_p,
                                                       uint32_t* s_cnt, double y, bool has_y, double* out, int32_t* pit) {
  const uint32_t tid = threadIdx.x, bs = blockDim.x, nw = bs >> 6;
  const uint32_t npairs = (n + 1u) / 2u;
  // 1. one transition of every pair over the record's dt, gamma and eta at the record's time, one observation draw
  for (uint32_t p = tid; p < npairs; p += bs) {
    const uint32_t ia = 2u * p, ib = ia + 1u;
    const bool hasb = ib < n;
    const uint32_t ja = s_anc[ia], jb = hasb ? s_anc[ib] : 0u;
    double xa[D], xb[D];
#pragma unroll
    for (int c = 0; c < D; ++c) { xa[c] = src[(size_t)c * n + ja]; xb[c] = hasb ? src[(size_t)c * n + jb] : 0.0; }
    if (hasb) propagate_pair<D>(mk, rec, rec->dt, key, (uint64_t)ia, 0u, tab, xa, xb);
    else propagate_one<D>(mk, rec, rec->dt, key, (uint64_t)ia, 0u, tab, xa);      // (the unpaired last particle of an odd cloud)
    {
      const double ea = link_of(mk.obs_kind, gamma_of<D>(mk, rec, xa));
      cssm_obs_stream sa = cssm_obs_stream_at(key, (uint64_t)ia, 0u);
      const double oa = cssm_obs_draw_one(&op, ea, &sa, tab);
#pragma unroll
      for (int c = 0; c < D; ++c) dst[(size_t)c * n + ia] = xa[c];
      stage[ia] = ea; stage[n + ia] = oa;
    }
    if (hasb) {
      const double eb = link_of(mk.obs_kind, gamma_of<D>(mk, rec, xb));
      cssm_obs_stream sb = cssm_obs_stream_at(key, (uint64_t)ib, 0u);
      const double ob = cssm_obs_draw_one(&op, eb, &sb, tab);
#pragma unroll
      for (int c = 0; c < D; ++c) dst[(size_t)c * n + ib] = xb[c];
      stage[ib] = eb; stage[n + ib] = ob;
    }
  }
  // 2. per row: the mean and the two order statistics, as k_fleet_forecast takes them
  for (uint32_t row = 0; row < (uint32_t)D + 2u; ++row) {
    __syncthreads();                                            // the record's values are written; the row before is read
    const double* v = (row < (uint32_t)D) ? dst + (size_t)row * n : stage + (size_t)(row - (uint32_t)D) * n;
    fleet_row_keys(v, n, np2, s_keys, s_p);
    fleet_sort_keys(s_keys, np2, tid, bs);
    __syncthreads();
    if (tid == 0) {
      double s = 0.0;
      for (uint32_t w = 0; w < nw; ++w) s += s_p[w];
      double* o = out + (size_t)row * 3u;
      o[0] = s / (double)n;
      o[1] = cssm_order_unkey(s_keys[row < (uint32_t)D ? rk.lo_state : rk.lo_eta]);
      o[2] = cssm_order_unkey(s_keys[row < (uint32_t)D ? rk.hi_state : rk.hi_eta]);
    }
  }
  // 3. the PIT counts (an extension: the reference has none): the draws strictly below / equal to the datum
  if (has_y) {                                                  // (uniform)
    uint32_t below = 0u, equal = 0u;
    for (uint32_t i = tid; i < n; i += bs) {
      const double o = stage[n + i];
      below += (o < y) ? 1u : 0u;
      equal += (o == y) ? 1u : 0u;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { below += __shfl_xor(below, off, 64); equal += __shfl_xor(equal, off, 64); }
    if ((tid & 63u) == 0u) { s_cnt[2u * (tid >> 6)] = below; s_cnt[2u * (tid >> 6) + 1u] = equal; }
    __syncthreads();
    if (tid == 0) {
      uint32_t b = 0u, e = 0u;
      for (uint32_t w = 0; w < nw; ++w) { b += s_cnt[2u * w]; e += s_cnt[2u * w + 1u]; }
      pit[0] = (int32_t)b; pit[1] = (int32_t)e;
    }
  }
  __syncthreads();                                              // dst, the keys and the waves' sums are free for the record's own step
}
