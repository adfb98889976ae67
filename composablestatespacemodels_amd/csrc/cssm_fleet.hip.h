// cssm_fleet.hip.h -- the fleet filter (include/cssm_pf.h, "fleet of independent series"): S small clouds of one model structure, ONE
// WORKGROUP PER SERIES.  A cloud of N <= CSSM_FLEET_MAX_N particles keeps its log-weights, its weights and its ancestors in the block's
// LDS, so nothing of a series ever crosses a block: no atomics on global memory, no flag another block waits for, no cooperative
// launch -- the parallelism of a launch is the number of series (grid.x = S).  k_fleet_series is instantiated per latent dimension in
// its own object (cssm_fleet_d.hip, -DCSSM_FLEET_D=d), as k_propagate is; cssm_fleet.hip holds the host side and k_fleet_summary.
//
// Every arithmetic statement of the contract is the existing device function: draw_normals / propagate_one, transition, gamma_of,
// logdens, cssm_ref_choose, cssm_exp_le0, cssm_fix_from_unit, wave_scan_u128, cssm_sys_count*, cssm_ess_of.  What is new here is only
// the order they run in and where their operands live.
#pragma once

#include "cssm_device.hip.h"

#define CSSM_FLEET_MAX_THREADS 512   /* 8 waves: two per SIMD, so every instantiation may use 256 vector registers */
#define CSSM_FLEET_WAVES(D) ((D) <= 4 ? 4 : 2)   /* waves per SIMD the register allocation aims at (the table and the A/B) */

#include "cssm_fleet_intervals.hip.h"
#include "cssm_fleet_onestep.hip.h"
#include "cssm_fleet_lgcp.hip.h"

// What the host uploads per (series, observation): the fields of cssm_build_rec's StepRec the kernels of a non-LGCP model read, with
// exactly the d components in use -- 80 + 40 d bytes (120 at d = 1, 200 at d = 3, 720 at d = 16) instead of sizeof(StepRec).  The
// block expands it into a StepRec in LDS, so the device functions above read it through the pointer they always took.
struct FleetRecHead {
  double y, c[4], cdf, u, dt, ref;
  int32_t has_obs;
  uint32_t step;
};   // followed by d x 4 transition coefficients (StepRec::coef) and d f coefficients (StepRec::fco)
#define CSSM_FLEET_REC_BYTES(d) (sizeof(FleetRecHead) + (size_t)(d) * 40u)

// per series, on the device: the Philox key and the initial-state parameters (x0 = sd0 z + m0) ...
struct FleetPar {
  uint64_t seed;
  double m0[CSSM_MAX_DIM], sd0[CSSM_MAX_DIM];
};
// ... and what a launch leaves for the next one and for the host
struct FleetSeries {
  double ll;
  int32_t ess;
  uint32_t err;        // bits 0 / 1 as Scalars::err: a NaN log-weight / no usable weight
  uint32_t fail_rec;   // index (within the launch's records of this series) of the observation that set err
  uint32_t pad_;
  double next_ref;     // (LGCP fleet) the level predicted for the series' NEXT event, cssm_ref_predict of the last event's max -- contract v8;
                       // NaN while the cloud has weighed none.  Every other launch writes NaN and reads nothing.
};

#define CSSM_FLEET_CTL_INIT 1u   /* draw the initial cloud before the series' first record of this launch */
#define CSSM_FLEET_CTL_BASE 2u   /* (RING) the series' window restarts: its first record of this launch also keeps the cloud it gathers */
#define CSSM_FLEET_CTL_FROM 4u   /* (with _INIT) the initial cloud is not drawn: particle i starts at a row of the caller's (FleetArgs::fr_*) */

// The window of cssm_fleet_step_interpolate (k_fleet_series<D, false, false, false, false, true> writes it, k_fleet_window reads it):
// per series `slices` clouds ([d][n] doubles each) and as many ancestor arrays ([n] each).  The host does the ring arithmetic: a kernel
// only ever sees slot numbers below `slices`.
struct FleetRing {
  double* x;                         // [S][slices][d][n]
  uint32_t* a;                       // [S][slices][n]
  const uint32_t* slot;              // per record of the launch: the slot that keeps the cloud the record writes and its ancestors
  const uint32_t* base;              // [S]: (CSSM_FLEET_CTL_BASE) the slot that keeps the cloud before the series' first record
  uint32_t slices;
};

struct FleetArgs {
  uint32_t n;                        // particles per series
  double* state;                     // [S][2][d][n]: record `step` reads buffer step & 1 and writes the other
  uint32_t* anc;                     // [S][n]
  FleetSeries* ser;                  // [S]
  const FleetPar* par;               // [S]
  const unsigned long long* off;     // [S + 1]: series k owns the launch's records off[k] .. off[k + 1] - 1
  const uint32_t* ctl;               // [S]: CSSM_FLEET_CTL_*
  const unsigned char* recs;         // compact records, CSSM_FLEET_REC_BYTES(d) each
  double* ll_t;                      // per record of the launch
  int32_t* ess_t;
  const double* logtab;
  ModelK mk;
  // `filter`'s sampled path (k_fleet_series<D, true> only; model/ParticleFilter.scala:152-158, Resampling.sampleOne).  Behind every
  // field the other instantiation reads: its kernel arguments stay where they were.
  const uint32_t* picks;             // per record of the launch: StepRec::pick, the slot sampleOne takes after that observation
  double* path;                      // may be null; series k owns rows off[k] + k .. off[k + 1] + k (T_k + 1 rows of d), preset to NaN
  double* last;                      // [S][d], preset to NaN: row T_k of series k's path
  // cssm_fleet_interpolate's forward pass (k_fleet_series<D, false, true> only), again behind every field the other instantiations read.
  // The launch's blocks are a CHUNK of series: off / recs / hser are the chunk's own (block b owns the records off[b] .. off[b + 1] - 1),
  // par is the fleet's (series k0 + b).  Block b keeps every cloud and every ancestor array of its series: slices off[b] + b .. off[b + 1]
  // + b of `hist` ([d][n] doubles each) and of `hanc` ([n] each) -- slice 0 the initial cloud, slice s + 1 the cloud record s wrote and
  // (behind a weighted record) the ancestors that resampled it.  state / anc / ser / ctl / ll_t / ess_t are not touched.
  double* hist;
  uint32_t* hanc;
  FleetSeries* hser;                 // [series of the chunk]: ll, err, fail_rec of the forward pass
  uint32_t k0;
  // getIntervals of the cloud behind the initial draw and behind every record (k_fleet_series<D, false, false, true> only:
  // cssm_fleet_filter_intervals / cssm_fleet_step_intervals; model/ParticleFilter.scala:415-424, examples/Filtering.scala:24-31), once
  // more behind every field the other instantiations read.
  const double* iv_fco0;             // [S][d]: F at series k's t0, the f coefficients of its row 0 (read by a launch that draws the cloud)
  double* iv_out;                    // rows of [d + 1][3] (mean, lower, upper), preset to NaN; iv_rows == 0: series k owns rows off[k] + k ..
                                     // off[k + 1] + k, row 0 the initial cloud; iv_rows == 1 (step): row k is the cloud behind series k's record;
                                     // iv_rows == 2 (a launch that continues: no initial cloud): row r is the cloud behind record r of the launch
  uint32_t iv_rows;
  uint32_t iv_np2;                   // the power of two >= max(n, 2): the keys a row's sort holds where the weights were
  FleetRowRanks iv_rk;
  // the one-step-ahead forecast of every record before it is stepped (k_fleet_series<D, false, false, false, true> only:
  // cssm_fleet_filter_forecasts / cssm_fleet_step_forecast; model/ParticleFilter.scala:368-409 over a filter stream), behind every field
  // the other instantiations read.  It takes iv_np2, iv_rk and iv_rows (1: the row of a record is its series' number) as IVAL does.
  FleetOneStep fc;
  // the window of cssm_fleet_step_interpolate (k_fleet_series<D, false, false, false, false, true> only), behind every field the other
  // instantiations read
  FleetRing ring;
  // an LGCP fleet's launch (k_fleet_series<D, PATH, false, false, false, false, true> only: cssm_fleet_lgcp.hip.h), behind every field the
  // other instantiations read.  `recs` are then FleetLgcpRecHead records, CSSM_FLEET_LGCP_REC_BYTES(d) each, and `picks` is not read.
  const double* fsub;                // the launch's sub-step table (f at the sub-step times of a seasonal leaf), or null: f is the record's own
  // the clouds of cssm_fleet_init_from (a series whose control word has CSSM_FLEET_CTL_FROM; FilterInit, model/ParticleFilter.scala:252-271),
  // behind every field the other launches read.  Series k owns the rows fr_moff[k] .. fr_moff[k + 1] - 1 of fr_x (d doubles each, M_k >= 1 of
  // them); particle i starts at row fr_pick[k n + i] of them, or without fr_pick at row cssm_posterior_pick(fr_keys[k], i, M_k) -- the
  // selection k_fleet_forecast_post makes; M_k = 1 reads neither.  fr_pick_out (may be null; [S][n]) receives the rows taken.
  const double* fr_x;
  const unsigned long long* fr_moff;
  const unsigned long long* fr_keys;
  const uint32_t* fr_pick;
  uint32_t* fr_pick_out;
};

// (IVAL) the row of FleetArgs::iv_out that receives the cloud behind record r of series k
__device__ __forceinline__ size_t fleet_iv_row_of(uint32_t iv_rows, uint32_t k, unsigned long long r) {
  return iv_rows == 1u ? (size_t)k : iv_rows == 2u ? (size_t)r : (size_t)(r + k + 1u);
}

// a - b mod 2^128 (integers: exact)
__device__ __forceinline__ cssm_u128 fleet_u128_sub(cssm_u128 a, cssm_u128 b) {
  cssm_u128 r;
  r.lo = a.lo - b.lo;
  r.hi = a.hi - b.hi - (a.lo < b.lo ? 1u : 0u);
  return r;
}

// cnt(C) of the contract for the cumulative sum `run` (include/cssm_numerics.h, systematic grid): the exact predicate, always
__device__ __forceinline__ uint32_t fleet_end_slot(cssm_u128 run, double totd, double u, uint32_t n, bool pow2, double inv_n) {
  const double C = cssm_u128_to_double(run) / totd;
  const uint32_t c = (uint32_t)(pow2 ? cssm_sys_count_pow2(C, u, n, inv_n) : cssm_sys_count(C, u, n));
  return (c > n) ? n : c;
}

// Row `row` of the series' sampled path: component tid of the particle in slot `pick` of the cloud in `buf`, through the ancestors
// (the identity behind the initial draw and behind an unweighted record).  The caller stands behind a barrier that completed both.
template <int D>
__device__ __forceinline__ void fleet_path_row(const double* buf, const uint32_t* s_anc, uint32_t n, uint32_t pick, double* row, uint32_t tid) {
  if (tid < (uint32_t)D) row[tid] = buf[(size_t)tid * n + s_anc[pick]];
}

// initialiseState of FilterInit (model/ParticleFilter.scala:258-262) and its posterior form: the cloud of a series from its M rows of the
// caller's (`rows`; FleetArgs::fr_*) into buffer 0, identity ancestors.  `pick` / `pick_out`: the series' own n entries, or null.  Called
// once per launch by a series that is started this way, before its records.
template <int D>
__device__ __forceinline__ void fleet_cloud_from(const double* rows, unsigned long long M, const uint32_t* pick, unsigned long long key,
                                                 uint32_t* pick_out, double* st, uint32_t* s_anc, uint32_t n, uint32_t tid, uint32_t bs) {
  for (uint32_t i = tid; i < n; i += bs) {
    const uint32_t p = (M == 1ull) ? 0u : (pick ? pick[i] : cssm_posterior_pick(key, (uint64_t)i, M));
    const double* row = rows + (size_t)p * D;
#pragma unroll
    for (int c = 0; c < D; ++c) st[(size_t)c * n + i] = row[c];
    if (pick_out) pick_out[i] = p;
    s_anc[i] = i;
  }
}

// llFilter / stepFilter of series blockIdx.x over its records of this launch (model/ParticleFilter.scala:105-140).
// Dynamic LDS: n_even doubles (log-weights, then the weights in their place) + n ancestors.
// PATH: `filter` (:152-158) -- a launch that draws the initial cloud also records one particle of it and one of the cloud after every
// record (FleetArgs::picks / path / last).  A template flag: the instantiation cssm_fleet_ll_filter and cssm_fleet_step run holds no
// trace of it (the resource table).
// HIST: the forward pass of cssm_fleet_interpolate (FilterInterpolate, model/ParticleFilter.scala:273-311) -- the same statements, but
// every cloud and every weighted record's ancestors are kept (FleetArgs::hist / hanc) instead of ping-ponging two buffers, and nothing
// the fleet holds per series is written.  A template flag as PATH is: the other two instantiations hold no trace of it either.
// IVAL: llFilter that also writes getIntervals of every cloud it passes through (FleetArgs::iv_*) -- fleet_cloud_intervals behind the
// barrier that completes the initial draw and behind the one that completes a record's cloud and ancestors, with the record's own f
// coefficients (s_rec.fco is F at the record's time).  The keys of a row's sort live where the weights were (dead once the resampling
// has read them), so the dynamic LDS is 8 np2 + 4 n bytes.  A template flag again: the other three instantiations hold no trace of it.
// FCST: llFilter that also forecasts every record just before it is stepped (FleetArgs::fc, cssm_fleet_onestep.hip.h) -- behind the
// barrier that completes the record in LDS: the cloud before the record through s_anc, one transition over the record's own dt and
// coefficients under the record's forecast key, into the record's destination buffer, which step 1 overwrites afterwards.  The keys of a
// row live where the weights were, as under IVAL (dead between a record's resampling and the next record's weighing).  A template flag
// once more: the other four instantiations hold no trace of it.
// RING: stepFilter that also remembers (FleetArgs::ring, cssm_fleet_step_interpolate) -- the cloud a record writes goes to the record's
// slot of the series' window as well as to its destination buffer, and behind the resampling (behind the None branch: with the
// identity) the ancestors go to the slot's ancestor slice; a series whose window restarts (CSSM_FLEET_CTL_BASE) keeps the cloud its first
// record gathers, not yet propagated, in its base slot.  The two cloud copies are loops of their own around step 1, which stays the
// plain launch's statement for statement.  state / anc / ser ping-pong as in the plain launch.  A template flag as the
// others: the other five instantiations hold no trace of it.
// LGCP: llFilter / stepFilter / filter of FilterLgcp (model/ParticleFilter.scala:169-227) -- every record is an event and is weighed.  The
// records are the LGCP fleet's own (FleetLgcpRecHead: no y, no density constants, sampleOne's slot inside); step 1 walks the event's n_sub
// sub-steps per particle (fleet_lgcp_weigh) instead of one transition and a density; the level is the one predicted from the series'
// event before (contract v8), kept in a register from record to record and in FleetSeries::next_ref from launch to launch.  Everything
// else -- the max, the fixed-point sums, the scan, the resampling -- is the plain launch's statement for statement.  A template flag as
// the others: the other six instantiations hold no trace of it.
template <int D, bool PATH, bool HIST = false, bool IVAL = false, bool FCST = false, bool RING = false, bool LGCP = false>
__global__ __launch_bounds__(CSSM_FLEET_MAX_THREADS, CSSM_FLEET_WAVES(D)) void k_fleet_series(const FleetArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char s_dyn[];
  __shared__ StepRec s_rec;
  __shared__ cssm_u128 s_wS[CSSM_FLEET_MAX_THREADS / 64], s_wS2[CSSM_FLEET_MAX_THREADS / 64];
  __shared__ unsigned long long s_wmax[CSSM_FLEET_MAX_THREADS / 64];
  __shared__ uint32_t s_wm[CSSM_FLEET_MAX_THREADS / 64], s_wbad[CSSM_FLEET_MAX_THREADS / 64];
  const uint32_t n = a.n, k = blockIdx.x, tid = threadIdx.x, bs = blockDim.x;
  const uint32_t lane = tid & 63u, wid = tid >> 6, nw = bs >> 6;
  double* s_lw = reinterpret_cast<double*>(s_dyn);
  uint32_t* s_anc = reinterpret_cast<uint32_t*>(s_dyn + (size_t)((IVAL || FCST) ? a.iv_np2 : ((n + 1u) & ~1u)) * 8u);
  const unsigned long long r0 = a.off[k], r1 = a.off[k + 1];
  const uint32_t ctl = HIST ? CSSM_FLEET_CTL_INIT : a.ctl[k];   // (HIST: a series is always run from its initial cloud)
  if ((HIST || !(ctl & CSSM_FLEET_CTL_INIT)) && r0 >= r1) return;   // (uniform) nothing for this series in this launch: untouched
  const double* tab = stage_log_table(a.logtab);
  const FleetPar* par = a.par + (HIST ? a.k0 + k : k);
  const uint64_t seed = par->seed;
  double* st = HIST ? a.hist + (size_t)(r0 + k) * D * n : a.state + (size_t)k * 2u * D * n;   // (HIST: slice 0 of the series)
  uint32_t* ganc = HIST ? a.hanc + (size_t)(r0 + k) * n : a.anc + (size_t)k * n;              // (HIST: ancestor slice 0, never written)
  double ll; int32_t ess; uint32_t err = 0u, fail_rec = 0u;
  double next_ref = cssm_nan();                                // (LGCP) no event of this cloud yet whose max could predict a level
  if (HIST || (ctl & CSSM_FLEET_CTL_INIT)) {
    // initialiseState (:105-108): x0 = sqrt(c0) z + m0 into buffer 0, identity ancestors, ll = 0, ess = N -- or (uniform) the caller's rows
    // (cssm_fleet_init_from launches the instantiation without a rider: the others hold no trace of its branch)
    if ((!PATH && !HIST && !IVAL && !FCST && !RING) && (ctl & CSSM_FLEET_CTL_FROM)) {
      const unsigned long long m0 = a.fr_moff[k];
      fleet_cloud_from<D>(a.fr_x + (size_t)m0 * D, a.fr_moff[k + 1] - m0, a.fr_pick ? a.fr_pick + (size_t)k * n : nullptr, a.fr_keys[k],
                          a.fr_pick_out ? a.fr_pick_out + (size_t)k * n : nullptr, st, s_anc, n, tid, bs);
    } else
    for (uint32_t i = tid; i < n; i += bs) {
      double z[D];
      draw_normals<D>(seed, (uint64_t)i, 0u, CSSM_STREAM_INIT, tab, z);
#pragma unroll
      for (int c = 0; c < D; ++c) st[(size_t)c * n + i] = par->sd0[c] * z[c] + par->m0[c];
      s_anc[i] = i;
    }
    ll = 0.0; ess = (int32_t)n;
  } else {
    for (uint32_t i = tid; i < n; i += bs) s_anc[i] = ganc[i];
    ll = a.ser[k].ll; ess = a.ser[k].ess;
    if constexpr (LGCP) next_ref = a.ser[k].next_ref;
  }
  const bool pow2 = (n & (n - 1u)) == 0u;
  const double inv_n = 1.0 / (double)n;
  const uint32_t it = (n + bs - 1u) / bs;                      // particles per thread of the scan phases (contiguous)
  const uint32_t j0 = tid * it;
  const uint32_t j1 = (j0 + it < n) ? j0 + it : n;             // (j0 >= n: an empty range)
  constexpr uint32_t RB = LGCP ? (uint32_t)CSSM_FLEET_LGCP_REC_BYTES(D) : (uint32_t)CSSM_FLEET_REC_BYTES(D);
  // (PATH) sampleOne's slot behind record q of the launch: the rider's array, or (LGCP) inside the record
  auto pick_of = [&](unsigned long long q) -> uint32_t {
    if constexpr (LGCP) return reinterpret_cast<const FleetLgcpRecHead*>(a.recs + (size_t)q * RB)->pick;
    else return a.picks[q];
  };
  uint32_t cur = 0u;                                           // (PATH) the buffer that holds the cloud: 0 behind the initial draw
  for (unsigned long long r = r0; r < r1; ++r) {               // bounded by the series' length
    __syncthreads();                                            // the cloud / ancestors of the record before; s_rec is free
    if (PATH && a.path) {                                       // (uniform) row r - r0: the initial cloud's pick, or the record before's
      uint32_t pick;
      if (r == r0) {
        const int32_t pr = (int32_t)cssm_philox_draw(seed, 0, 0, CSSM_STREAM_PICK, 0).v[0];
        pick = (uint32_t)((uint64_t)(pr < 0 ? (uint32_t)0 - (uint32_t)pr : (uint32_t)pr) % n);
      } else {
        pick = pick_of(r - 1);
      }
      fleet_path_row<D>(st + (size_t)cur * D * n, s_anc, n, pick, a.path + (size_t)(r + k) * D, tid);
    }
    if (IVAL && r == r0 && (ctl & CSSM_FLEET_CTL_INIT))         // (uniform) row 0: the initial cloud, F at the series' t0
      fleet_cloud_intervals<D>(st, s_anc, n, a.iv_np2, a.mk, a.iv_fco0 + (size_t)k * D, a.iv_rk, reinterpret_cast<unsigned long long*>(s_lw),
                               a.iv_out + (size_t)(r0 + k) * (D + 1) * 3u);
    if constexpr (LGCP) {
      const unsigned char* g = a.recs + (size_t)r * RB;
      const FleetLgcpRecHead* h = reinterpret_cast<const FleetLgcpRecHead*>(g);
      const double* tail = reinterpret_cast<const double*>(g + sizeof(FleetLgcpRecHead));
      if (tid == 0) {
        s_rec.u = h->u; s_rec.dt = h->dt; s_rec.n_sub = h->n_sub; s_rec.step = h->step; s_rec.fsub_off = h->fsub_off; s_rec.has_obs = 1;
      }
      if (tid < 4u * D) s_rec.coef[tid >> 2][tid & 3u] = tail[tid];
      if (tid < (uint32_t)D) s_rec.fco[tid] = tail[4 * D + tid];
    } else {
      const unsigned char* g = a.recs + (size_t)r * RB;
      const FleetRecHead* h = reinterpret_cast<const FleetRecHead*>(g);
      const double* tail = reinterpret_cast<const double*>(g + sizeof(FleetRecHead));
      if (tid == 0) {
        s_rec.y = h->y; s_rec.c[0] = h->c[0]; s_rec.c[1] = h->c[1]; s_rec.c[2] = h->c[2]; s_rec.c[3] = h->c[3];
        s_rec.cdf = h->cdf; s_rec.u = h->u; s_rec.dt = h->dt; s_rec.ref = h->ref; s_rec.has_obs = h->has_obs; s_rec.step = h->step;
      }
      if (tid < 4u * D) s_rec.coef[tid >> 2][tid & 3u] = tail[tid];
      if (tid < (uint32_t)D) s_rec.fco[tid] = tail[4 * D + tid];
    }
    __syncthreads();
    const StepRec* rec = &s_rec;
    const uint32_t step = rec->step;
    const bool weighted = LGCP || rec->has_obs != 0;
    const double* src = st + (size_t)(HIST ? (uint32_t)(r - r0) : (step & 1u)) * D * n;
    double* dst = st + (size_t)(HIST ? (uint32_t)(r - r0) + 1u : ((step & 1u) ^ 1u)) * D * n;
    if (PATH) cur = (step & 1u) ^ 1u;
    if constexpr (FCST) {                                       // (uniform) the forecast of this record from the cloud before it
      __shared__ double s_fcp[CSSM_FLEET_MAX_THREADS / 64];     // the waves' partial sums of a row's mean ...
      __shared__ uint32_t s_fcc[2 * (CSSM_FLEET_MAX_THREADS / 64)];   // ... and their PIT counts
      const uint32_t fl = a.fc.flags[r];
      if (fl & CSSM_FLEET_FC_ON) {
        const size_t row = a.iv_rows ? (size_t)k : (size_t)r;
        fleet_onestep_forecast<D>(a.mk, rec, src, dst, s_anc, n, a.iv_np2, a.fc.keys[r], a.fc.op[k], a.fc.stage + (size_t)k * 2u * n, tab, a.iv_rk,
                                  reinterpret_cast<unsigned long long*>(s_lw), s_fcp, s_fcc, a.fc.y[r], (fl & CSSM_FLEET_FC_HAS) != 0u,
                                  a.fc.out + row * (D + 2) * 3u, a.fc.pit + row * 2u);
      }
    }
    // (RING) the record's slot of the series' window, and the base slot of a window that restarts at this record
    double* ring_x = nullptr; uint32_t* ring_a = nullptr; double* ring_b = nullptr;
    if constexpr (RING) {
      const size_t w0 = (size_t)k * a.ring.slices, sl = w0 + a.ring.slot[r];
      ring_x = a.ring.x + sl * D * n; ring_a = a.ring.a + sl * n;
      if (r == r0 && (ctl & CSSM_FLEET_CTL_BASE)) ring_b = a.ring.x + (w0 + a.ring.base[k]) * D * n;
      if (ring_b) {                                             // (uniform) X[anc[i]], not yet propagated: what cssm_fleet_get_particles returns
        for (uint32_t i = tid; i < n; i += bs) {
          const uint32_t j = s_anc[i];
#pragma unroll
          for (int c = 0; c < D; ++c) ring_b[(size_t)c * n + i] = src[(size_t)c * n + j];
        }
      }
    }
    // 1. gather through the previous ancestors, transition, f, log-density (:118, :123)
    double tmax = -cssm_inf();
    bool bad = false;
    if constexpr (LGCP) {
      // (LGCP) 1. gather through the previous ancestors, the event's sub-steps, gamma - hazard (:193-205, :212-217).  W of the thread's
      //    particles at a time (cssm_fleet_lgcp.hip.h); a lane whose group is short walks its first particle again and stores nothing of it
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
        fleet_lgcp_weigh<D, W>(a.mk, rec, a.fsub, seed, gid, tab, x, lw);
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
    } else
    for (uint32_t i = tid; i < n; i += bs) {
      const uint32_t j = s_anc[i];
      double x[D];
#pragma unroll
      for (int c = 0; c < D; ++c) x[c] = src[(size_t)c * n + j];
      propagate_one<D>(a.mk, rec, rec->dt, seed, (uint64_t)i, step, tab, x);
#pragma unroll
      for (int c = 0; c < D; ++c) dst[(size_t)c * n + i] = x[c];
      if (weighted) {
        double lw = logdens<-1>(a.mk, rec, gamma_of<D>(a.mk, rec, x), tab);
        if (lw != lw) { bad = true; lw = -cssm_inf(); }
        tmax = (lw > tmax) ? lw : tmax;
        s_lw[i] = lw;
      }
    }
    if constexpr (RING) {                                       // the cloud this record wrote, into its slot: a thread copies the particles it wrote itself
      for (uint32_t i = tid; i < n; i += bs) {
#pragma unroll
        for (int c = 0; c < D; ++c) ring_x[(size_t)c * n + i] = dst[(size_t)c * n + i];
      }
    }
    if (!weighted) {                                            // (uniform) the None branch (:121): the cloud moves, nothing else
      __syncthreads();
      for (uint32_t i = tid; i < n; i += bs) {
        s_anc[i] = i;
        if constexpr (RING) ring_a[i] = i;
      }
      if (!HIST && tid == 0) { a.ll_t[r] = ll; a.ess_t[r] = ess; }
      if (IVAL) {                                               // the cloud this record moved, through identity ancestors
        __syncthreads();
        fleet_cloud_intervals<D>(dst, s_anc, n, a.iv_np2, a.mk, s_rec.fco, a.iv_rk, reinterpret_cast<unsigned long long*>(s_lw),
                                 a.iv_out + fleet_iv_row_of(a.iv_rows, k, r) * (D + 1) * 3u);
      }
      continue;
    }
    // 2. the block's own max is at hand before any weight is formed: the level is chosen in place
    {
      const unsigned long long km = wave_max_u64(cssm_order_key(tmax));
      const bool anyb = __any(bad);
      if (lane == 0u) { s_wmax[wid] = km; s_wbad[wid] = anyb ? 1u : 0u; }
    }
    __syncthreads();
    unsigned long long kmax = 0ull; uint32_t anybad = 0u;
    for (uint32_t w = 0; w < nw; ++w) { kmax = (s_wmax[w] > kmax) ? s_wmax[w] : kmax; anybad |= s_wbad[w]; }
    const double gmax = cssm_order_unkey(kmax);
    if (anybad || !(gmax > -cssm_inf()) || !(gmax < cssm_inf())) {   // (uniform) unusable weights: the series is over
      err = anybad ? 1u : 2u; fail_rec = (uint32_t)(r - r0);
      break;
    }
    double ref;
    if constexpr (LGCP) {                                       // the level predicted from the event before; this event's max predicts the next
      ref = cssm_ref_choose(next_ref, gmax);
      next_ref = cssm_ref_predict(gmax);
    } else {
      ref = cssm_ref_choose(rec->ref, gmax);
    }
    // 3. weights on the 2^-96 grid, their sums, the block scan (:125, :127-128)
    cssm_u128 sa = cssm_u128_zero(), sb = cssm_u128_zero();
    for (uint32_t j = j0; j < j1; ++j) {
      const double w1 = cssm_exp_le0(cssm_min_c(s_lw[j] - ref, CSSM_REF_BELOW));
      s_lw[j] = w1;
      sa = cssm_u128_add(sa, cssm_fix_from_unit(w1));
      sb = cssm_u128_add(sb, cssm_fix_from_unit(w1 * w1));
    }
    for (uint32_t i = tid; i < n; i += bs) s_anc[i] = 0u;      // (every thread gathered before the barrier above)
    const cssm_u128 inc = wave_scan_u128(sa, (int)lane);
    const cssm_u128 wb2 = wave_sum_u128(sb);
    if (lane == 63u) { s_wS[wid] = inc; s_wS2[wid] = wb2; }
    __syncthreads();
    cssm_u128 tot = cssm_u128_zero(), tot2 = cssm_u128_zero(), off = cssm_u128_zero();
    for (uint32_t w = 0; w < nw; ++w) {
      if (w < wid) off = cssm_u128_add(off, s_wS[w]);
      tot = cssm_u128_add(tot, s_wS[w]); tot2 = cssm_u128_add(tot2, s_wS2[w]);
    }
    if (cssm_u128_is_zero(tot)) { err = 2u; fail_rec = (uint32_t)(r - r0); break; }   // (uniform)
    ll = ll + ref + cssm_log(cssm_fix_to_double(tot) / (double)n);
    ess = cssm_ess_of(tot, tot2);
    // 4. systematic resampling (model/Resampling.scala:36-72): particle j owns the slots [cnt(C_{j-1}), cnt(C_j)); it drops its
    //    index at the first of them, an inclusive max-scan over the slots fills the runs (indices grow with the slots; an empty
    //    slot reads 0, which is also particle 0's marker: the slots before every other marker can only be its run)
    {
      const double totd = cssm_u128_to_double(tot);
      const double u = rec->u;
      cssm_u128 run = fleet_u128_sub(cssm_u128_add(off, inc), sa);   // exclusive prefix of the thread's first particle
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
      uint32_t m = 0u;
      for (uint32_t s = j0; s < j1; ++s) { const uint32_t v = s_anc[s]; m = (v > m) ? v : m; }
      const uint32_t incl = wave_scan_max_u32(m);
      uint32_t carry = dpp0<0x138 /* wave_shr:1 */, 0xf>(incl);
      if (lane == 63u) s_wm[wid] = incl;
      __syncthreads();
      for (uint32_t w = 0; w < wid; ++w) carry = (s_wm[w] > carry) ? s_wm[w] : carry;
      uint32_t* hslice = HIST ? ganc + (size_t)((uint32_t)(r - r0) + 1u) * n : nullptr;   // (HIST) the ancestors that resampled slice s + 1
      for (uint32_t s = j0; s < j1; ++s) {
        const uint32_t v = s_anc[s];
        carry = (v > carry) ? v : carry;
        s_anc[s] = carry;
        if (HIST) hslice[s] = carry;
        if constexpr (RING) ring_a[s] = carry;
      }
    }
    if (!HIST && tid == 0) { a.ll_t[r] = ll; a.ess_t[r] = ess; }
    if (IVAL) {                                                 // the cloud this record wrote, through the ancestors that resampled it
      __syncthreads();
      fleet_cloud_intervals<D>(dst, s_anc, n, a.iv_np2, a.mk, s_rec.fco, a.iv_rk, reinterpret_cast<unsigned long long*>(s_lw),
                               a.iv_out + fleet_iv_row_of(a.iv_rows, k, r) * (D + 1) * 3u);
    }
  }
  if (HIST) {                                                   // the fleet's ancestors and scalars stay as they were
    if (tid == 0) { FleetSeries o; o.ll = ll; o.ess = ess; o.err = err; o.fail_rec = fail_rec; o.pad_ = 0u; o.next_ref = cssm_nan(); a.hser[k] = o; }
    return;
  }
  __syncthreads();
  if (PATH && !err && r1 > r0) {                               // (uniform) the last row: no record follows to write it
    const uint32_t pick = pick_of(r1 - 1);
    if (a.path) fleet_path_row<D>(st + (size_t)cur * D * n, s_anc, n, pick, a.path + (size_t)(r1 + k) * D, tid);
    fleet_path_row<D>(st + (size_t)cur * D * n, s_anc, n, pick, a.last + (size_t)k * D, tid);
  }
  for (uint32_t i = tid; i < n; i += bs) ganc[i] = s_anc[i];
  if (tid == 0) { FleetSeries o; o.ll = ll; o.ess = ess; o.err = err; o.fail_rec = fail_rec; o.pad_ = 0u; o.next_ref = next_ref; a.ser[k] = o; }
}

// which k_fleet_series a launch runs: <D, false> | <D, true> | <D, false, true> | <D, false, false, true> | <D, false, false, false, true> |
// <D, false, false, false, false, true>
enum class FleetKind : int { plain, path, hist, ival, fcst, ring };
struct FleetLaunch {
  FleetArgs args;
  uint32_t n_series;    // blocks; hist: the series args.k0 .. args.k0 + n_series - 1
  FleetKind kind;
  bool lgcp;            // an LGCP fleet's launch: kind plain or path runs <D, false / true, false, false, false, false, true>
  int threads;
  size_t lds;           // ival, fcst: 8 args.iv_np2 + 4 n bytes
  hipStream_t stream;
};
// one per latent dimension, defined in cssm_fleet_d.hip
#define CSSM_DECL_FLEET(D) int cssm_fleet_launch_d##D(const FleetLaunch& l);
CSSM_DECL_FLEET(1) CSSM_DECL_FLEET(2) CSSM_DECL_FLEET(3) CSSM_DECL_FLEET(4) CSSM_DECL_FLEET(5) CSSM_DECL_FLEET(6) CSSM_DECL_FLEET(7) CSSM_DECL_FLEET(8)
CSSM_DECL_FLEET(9) CSSM_DECL_FLEET(10) CSSM_DECL_FLEET(11) CSSM_DECL_FLEET(12) CSSM_DECL_FLEET(13) CSSM_DECL_FLEET(14) CSSM_DECL_FLEET(15) CSSM_DECL_FLEET(16)
#undef CSSM_DECL_FLEET
