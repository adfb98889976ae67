// cssm_fleet_forecast.hip -- forecasts of every series of a fleet in ONE launch (include/cssm_pf.h: cssm_fleet_forecast,
// cssm_fleet_forecast_posterior): the scan of SimulateData.forecast + summariseForecast (model/Data.scala:196-231,
// model/ParticleFilter.scala:368-409) per series, ONE WORKGROUP PER SERIES as k_fleet_series.  A block runs the whole chain of its
// series' horizons: nothing of a series crosses a block -- no atomics on global memory, no flag another block reads, no cooperative
// launch; every loop is bounded by N or by the series' horizons.
//
// All of that is fleet_forecast_body<D, Src>, written once.  The two kernels are entry points that fill a source and call it:
// k_fleet_forecast<D> with FleetCloudSrc (the series' cloud through its ancestors, moved under the series' records) and
// k_fleet_forecast_post<D> with FleetPostSrc (a pair of the series' posterior sample per particle: its state, its own parameters).
// A source says where a pair starts, what moves it one step and which observation parameters each particle draws with -- the split
// of forecast_body<D, Src> (cssm_forecast.hip) for the single handle.
//
// Every arithmetic statement is the existing device function, so a series has the bits of cssm_pf_forecast /
// cssm_pf_forecast_posterior on a handle of its own: propagate_pair / propagate_one, or post_step (cssm_posterior_move.hip.h) -- the
// paired CSSM_STREAM_STEP streams under the forecast's key at step h --, gamma_of, link_of, cssm_obs_draw_one on cssm_obs_stream_at
// (CSSM_STREAM_OBS), cssm_order_key; the ranks are sel_ranks' (the host passes them).  The order statistics of a row are exact either
// way: k_fleet_summary's bitonic network over the row's keys in LDS, or (FleetFcArgs::select) a radix select over them in LDS, the
// single handle's k_sel_hist / k_sel_pick in one block; the means are plain fp64 sums.
//
// Where the operands live.  Horizon 0 gathers from the source (the series' cloud in buffer step & 1 through its ancestors, or the
// posterior states x[pick_i]); the states between horizons live in the series' OTHER state buffer, which is free between calls -- the
// next record of k_fleet_series overwrites all of it before anything reads it (a series without a cloud lends buffer 1).  A thread
// always owns the same particle pairs, so it updates them in place without a barrier.  eta and the observation draw of a horizon are
// staged in 2 N doubles of per-series scratch (written and read by the same block), so the block's LDS holds one row of keys only and
// as many blocks fit a CU as k_fleet_summary's.
#include <hip/hip_runtime.h>

#include "cssm_internal.h"
#include "cssm_kernels.hip.h"
#include "cssm_posterior_move.hip.h"
#include "cssm_fleet_forecast.hip.h"

// What the two fleet forecasts share -- everything but where a pair starts and what moves it.  A source `s` answers: series (what it
// needs of series k before the first horizon), pair (what it needs of the pair (ia, ib) at a horizon, before any load), x0 (the pair's
// states before the first horizon), step (one transition of the pair, or of its first particle alone) and obs (the observation
// parameters particle b of the pair draws with).
template <int D, class Src>
__device__ __forceinline__ void fleet_forecast_body(const FleetFcArgs& a, Src& s) {
  extern __shared__ unsigned long long s_keys[];
  __shared__ StepRec s_rec;
  __shared__ double s_p[CSSM_FLEET_MAX_THREADS / 64];
  __shared__ uint32_t s_h[2][256];                             // radix select: the digit counts of the two targets
  __shared__ unsigned long long s_pre[2];                      // ... the digits found so far
  __shared__ uint32_t s_rk[2];                                 // ... the rank among the keys that share them
  const uint32_t n = a.n, np2 = a.np2, k = a.k0 + blockIdx.x, tid = threadIdx.x, bs = blockDim.x;
  const unsigned long long r0 = a.off[k], r1 = a.off[k + 1];
  const uint32_t cur = a.cur[k];
  if (r0 >= r1 || cur > 1u) return;                            // (uniform) no horizons, or the host refused the series: untouched
  const double* tab = stage_log_table(a.logtab);
  const uint64_t key = a.keys[k];
  double* st = a.state + (size_t)k * 2u * D * n;
  double* wrk = st + (size_t)(cur ^ 1u) * D * n;               // the states between horizons
  s.series(a, k, st + (size_t)cur * D * n);
  double* stage = a.stage + (size_t)k * 2u * n;                // eta[n], obs[n] of the horizon at hand
  const uint32_t npairs = (n + 1u) / 2u, nw = bs >> 6;
  constexpr uint32_t RB = (uint32_t)CSSM_FLEET_REC_BYTES(D);
  for (unsigned long long r = r0; r < r1; ++r) {               // bounded by the series' horizons
    __syncthreads();                                            // the row sorted last; s_rec is free
    {
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
    const uint32_t h = rec->step;                               // the horizon's index: the Philox counter word of both streams
    const bool first = r == r0;
    double* smp = a.samples ? a.samples + (size_t)(r - a.samp_r0) * (D + 3) * n : nullptr;
    // 1. one transition of every pair, gamma and eta at t[h], one observation draw
    for (uint32_t p = tid; p < npairs; p += bs) {
      const uint32_t ia = 2u * p, ib = ia + 1u;
      const bool hasb = ib < n;
      double xa[D], xb[D];
      s.pair(first, hasb, ia, ib, key);
      if (first) {
        s.x0(hasb, ia, ib, n, xa, xb);
      } else {
#pragma unroll
        for (int c = 0; c < D; ++c) { xa[c] = wrk[(size_t)c * n + ia]; xb[c] = hasb ? wrk[(size_t)c * n + ib] : 0.0; }
      }
      s.step(hasb, a.mk, rec, key, (uint64_t)ia, h, tab, xa, xb);
      {
        const double ga = gamma_of<D>(a.mk, rec, xa);
        const double ea = link_of(a.mk.obs_kind, ga);
        cssm_obs_stream sa = cssm_obs_stream_at(key, (uint64_t)ia, h);
        const double oa = cssm_obs_draw_one(&s.obs(0), ea, &sa, tab);
#pragma unroll
        for (int c = 0; c < D; ++c) wrk[(size_t)c * n + ia] = xa[c];
        stage[ia] = ea; stage[n + ia] = oa;
        if (smp) {   // rows of a horizon: state..., gamma, eta, obs
#pragma unroll
          for (int c = 0; c < D; ++c) smp[(size_t)c * n + ia] = xa[c];
          smp[(size_t)D * n + ia] = ga; smp[(size_t)(D + 1) * n + ia] = ea; smp[(size_t)(D + 2) * n + ia] = oa;
        }
      }
      if (hasb) {
        const double gb = gamma_of<D>(a.mk, rec, xb);
        const double eb = link_of(a.mk.obs_kind, gb);
        cssm_obs_stream sb = cssm_obs_stream_at(key, (uint64_t)ib, h);
        const double ob = cssm_obs_draw_one(&s.obs(1), eb, &sb, tab);
#pragma unroll
        for (int c = 0; c < D; ++c) wrk[(size_t)c * n + ib] = xb[c];
        stage[ib] = eb; stage[n + ib] = ob;
        if (smp) {
#pragma unroll
          for (int c = 0; c < D; ++c) smp[(size_t)c * n + ib] = xb[c];
          smp[(size_t)D * n + ib] = gb; smp[(size_t)(D + 1) * n + ib] = eb; smp[(size_t)(D + 2) * n + ib] = ob;
        }
      }
    }
    // 2. per row: the mean and the two order statistics (k_fleet_summary's network: the next power of two, padded with the largest key)
    for (uint32_t row = 0; row < (uint32_t)D + 2u; ++row) {
      __syncthreads();                                          // the horizon's values are written; the row before is read
      const double* v = (row < (uint32_t)D) ? wrk + (size_t)row * n : stage + (size_t)(row - (uint32_t)D) * n;
      fleet_row_keys(v, n, np2, s_keys, s_p);
      const uint32_t lo = row < (uint32_t)D ? a.lo_state : a.lo_eta, hi = row < (uint32_t)D ? a.hi_state : a.hi_eta;
      unsigned long long klo, khi;
      if (a.select) {                                           // (uniform)
        // exact radix select, most significant byte first, both targets at once (k_sel_hist / k_sel_pick of the single handle, in
        // LDS): per byte the counts of the keys that share the digits found so far, then wave 0 finds the digit that holds the rank
        for (uint32_t i = tid; i < 512u; i += bs) (&s_h[0][0])[i] = 0u;
        if (tid < 2u) { s_pre[tid] = 0ull; s_rk[tid] = tid ? hi : lo; }
        for (int shift = 56; shift >= 0; shift -= 8) {          // eight passes
          __syncthreads();                                      // the keys; the counts are zero; the digits of the pass before
          const unsigned long long p0 = s_pre[0], p1 = s_pre[1];
          const unsigned long long hm = (shift >= 56) ? 0ull : (~0ull << (shift + 8));   // bits above the current byte
          for (uint32_t i = tid; i < n; i += bs) {
            const unsigned long long kk = s_keys[i];
            const uint32_t b = (uint32_t)(kk >> shift) & 255u;
            if ((kk & hm) == (p0 & hm)) atomicAdd(&s_h[0][b], 1u);
            if ((kk & hm) == (p1 & hm)) atomicAdd(&s_h[1][b], 1u);
          }
          __syncthreads();
          if (tid < 64u) {                                      // four digits per lane; the lane whose digits hold the rank walks them
#pragma unroll
            for (int q = 0; q < 2; ++q) {
              uint32_t c[4];
#pragma unroll
              for (int m = 0; m < 4; ++m) { c[m] = s_h[q][4u * tid + m]; s_h[q][4u * tid + m] = 0u; }
              const uint32_t tot = c[0] + c[1] + c[2] + c[3];
              uint32_t incl = tot;
#pragma unroll
              for (int off = 1; off < 64; off <<= 1) { const uint32_t up = __shfl_up(incl, off, 64); if (tid >= (uint32_t)off) incl += up; }
              const uint32_t rk = s_rk[q];
              uint32_t cum = incl - tot;
              if (rk >= cum && rk < incl) {
                uint32_t b = 4u * tid;
#pragma unroll
                for (int m = 0; m < 3; ++m) if (b == 4u * tid + m && cum + c[m] <= rk) { cum += c[m]; ++b; }
                s_pre[q] |= (unsigned long long)b << shift;
                s_rk[q] = rk - cum;
              }
            }
          }
        }
        __syncthreads();
        klo = s_pre[0]; khi = s_pre[1];
      } else {
        fleet_sort_keys(s_keys, np2, tid, bs);
        __syncthreads();
        klo = s_keys[lo]; khi = s_keys[hi];
      }
      if (tid == 0) {
        double s = 0.0;
        for (uint32_t w = 0; w < nw; ++w) s += s_p[w];
        double* o = a.out + ((size_t)r * (D + 2) + row) * 3u;
        o[0] = s / (double)n;
        o[1] = cssm_order_unkey(klo);
        o[2] = cssm_order_unkey(khi);
      }
    }
  }
}

// Source 1: the series' cloud under the series' records.  A pair is gathered through the ancestors and moves by propagate_pair (the
// unpaired last particle of an odd cloud: propagate_one); both particles draw with the series' one set of observation parameters.
template <int D>
struct FleetCloudSrc {
  const double* src; const uint32_t* ganc;
  cssm_obs_params op;
  __device__ __forceinline__ void series(const FleetFcArgs& a, uint32_t k, const double* cloud) {
    op = a.op[k]; src = cloud; ganc = a.anc + (size_t)k * a.n;
  }
  __device__ __forceinline__ void pair(bool, bool, uint32_t, uint32_t, uint64_t) {}
  __device__ __forceinline__ void x0(bool hasb, uint32_t ia, uint32_t ib, uint32_t n, double (&xa)[D], double (&xb)[D]) const {
    const uint32_t ja = ganc[ia], jb = hasb ? ganc[ib] : 0u;
#pragma unroll
    for (int c = 0; c < D; ++c) { xa[c] = src[(size_t)c * n + ja]; xb[c] = hasb ? src[(size_t)c * n + jb] : 0.0; }
  }
  __device__ __forceinline__ void step(bool hasb, const ModelK& mk, const StepRec* rec, uint64_t key, uint64_t ia, uint32_t h, const double* tab,
                                       double (&xa)[D], double (&xb)[D]) const {
    if (hasb) propagate_pair<D>(mk, rec, rec->dt, key, ia, h, tab, xa, xb);
    else propagate_one<D>(mk, rec, rec->dt, key, ia, h, tab, xa);      // (the unpaired last particle of an odd cloud)
  }
  __device__ __forceinline__ const cssm_obs_params& obs(int) const { return op; }
};

template <int D>
__global__ __launch_bounds__(CSSM_FLEET_MAX_THREADS, CSSM_FLEET_WAVES(D)) void k_fleet_forecast(const FleetFcArgs a) {
  FleetCloudSrc<D> s;
  fleet_forecast_body<D>(a, s);
}

// Source 2: a pair of the series' posterior sample per particle (PostSrc of cssm_forecast.hip, per series).  Series k owns the pairs
// moff[k] .. moff[k + 1] - 1 of x (M x D) and rows (M x (3 D + 1): the parameter set, then the observation constant p0).  Particle i
// sits on pair pick_i of its series: picks[k][i] as the host uploaded it, or (draw) cssm_posterior_pick(keys[k], i, M_k), which the
// first horizon writes there -- the later horizons and the host read it back (a thread always owns the same pairs: no barrier).  A
// thread serves several pairs per horizon, so a pair's parameters are loaded at every horizon; of a record only dt and the f
// coefficients are used.
template <int D>
struct FleetPostSrc {
  static constexpr size_t S = 3 * D + 1;
  const FleetFcPost q;
  const double* x; const double* rows; uint32_t* picks; uint32_t M;
  cssm_obs_params opa, opb;   // (kind and df: the model's; p0: the particle's row)
  uint32_t ma, mb;
  PostParams<D, (D <= CSSM_FLEET_POST_REG_MAX_D)> pa, pb;
  __device__ __forceinline__ explicit FleetPostSrc(const FleetFcPost& q_) : q(q_) {}
  __device__ __forceinline__ void series(const FleetFcArgs& a, uint32_t k, const double*) {
    const unsigned long long m0 = q.moff[k];
    M = (uint32_t)(q.moff[k + 1] - m0);
    x = q.x + (size_t)m0 * D; rows = q.rows + (size_t)m0 * S; picks = q.picks + (size_t)k * a.n;
    opa.kind = opb.kind = a.mk.obs_kind; opa.df = opb.df = q.obs_df;
  }
  __device__ __forceinline__ void pair(bool first, bool hasb, uint32_t ia, uint32_t ib, uint64_t key) {
    if (first && q.draw) {
      ma = cssm_posterior_pick(key, (uint64_t)ia, (uint64_t)M); mb = hasb ? cssm_posterior_pick(key, (uint64_t)ib, (uint64_t)M) : 0u;
      picks[ia] = ma;
      if (hasb) picks[ib] = mb;
    } else {
      ma = picks[ia]; mb = hasb ? picks[ib] : 0u;
    }
    pa.load(rows + (size_t)ma * S);
    pb.load(rows + (size_t)mb * S);
    opa.p0 = rows[(size_t)ma * S + 3 * D];
    opb.p0 = rows[(size_t)mb * S + 3 * D];
  }
  __device__ __forceinline__ void x0(bool hasb, uint32_t, uint32_t, uint32_t, double (&xa)[D], double (&xb)[D]) const {
#pragma unroll
    for (int c = 0; c < D; ++c) { xa[c] = x[(size_t)ma * D + c]; xb[c] = hasb ? x[(size_t)mb * D + c] : 0.0; }
  }
  __device__ __forceinline__ void step(bool hasb, const ModelK& mk, const StepRec* rec, uint64_t key, uint64_t ia, uint32_t h, const double* tab,
                                       double (&xa)[D], double (&xb)[D]) const {
    post_step<D>(hasb, mk, rec->dt, key, ia, h, tab, pa, pb, xa, xb);
  }
  __device__ __forceinline__ const cssm_obs_params& obs(int b) const { return b ? opb : opa; }
};

template <int D>
__global__ __launch_bounds__(CSSM_FLEET_MAX_THREADS, CSSM_FLEET_WAVES(D)) void k_fleet_forecast_post(const FleetFcArgs a, const FleetFcPost q) {
  FleetPostSrc<D> s(q);
  fleet_forecast_body<D>(a, s);
}

int cssm_fleet_forecast_launch(const FleetFcLaunch& l) {
  DISPATCH_D(l.d, hipLaunchKernelGGL(k_fleet_forecast<D>, dim3(l.n_series), dim3(l.threads), (size_t)l.args.np2 * 8u, l.stream, l.args));
  return (int)hipGetLastError();
}

int cssm_fleet_forecast_post_launch(const FleetFcLaunch& l, const FleetFcPost& q) {
  DISPATCH_D(l.d, hipLaunchKernelGGL(k_fleet_forecast_post<D>, dim3(l.n_series), dim3(l.threads), (size_t)l.args.np2 * 8u, l.stream, l.args, q));
  return (int)hipGetLastError();
}
