// cssm_forecast.hip -- forecasts from the filtered cloud: ParticleFilter.getForecast / getMeanForecast (model/ParticleFilter.scala:
// 368-409) and the scan of SimulateData.forecast + summariseForecast over future times (model/Data.scala:196-231), and the stateless
// observation draw on given etas (cssm_obs_draw).  See include/cssm_pf.h for the contract, include/cssm_obs_draws.h for the draws.
//
// One call = chunks of horizons.  Per chunk: the forecast kernel (one thread per particle PAIR, so that every Philox block of the
// transition serves both particles, as in k_propagate) gathers the pair once -- from its source, or from the carry buffer of the
// chunk before -- and runs the chunk's horizons with the state in registers: transition (CSSM_STREAM_STEP under `key` at step h),
// gamma and eta at t[h], one observation draw (CSSM_STREAM_OBS), the d + 2 order keys and the block's fp64 partial sums per horizon.
// Then one radix selection (k_sel_hist / k_sel_pick, grid.y = the chunk's rows) and k_forecast_finish (means and the order
// statistics per row).  The filter's own buffers are only read.
//
// All of that is forecast_body<D, Src>, written once.  The two kernels are entry points that fill a source and call it:
// k_forecast<D> with CloudSrc (the handle's current cloud through the indirection k_summary_fill reads, moved under the handle's
// records) and k_forecast_post<D> with PostSrc (a pair of a posterior sample per particle: its state, its own parameters).  A source
// says where a particle starts, what moves a pair one step and which observation parameters each particle draws with; both step
// whole pairs through pair_normals_feed and a component through transition_step (cssm_posterior_move.hip.h, cssm_device.hip.h).
// A third entry point, k_forecast_row<D>, is the body with the compile-time flag ROW over CloudSrc: the first launch of a row of
// cssm_pf_filter_forecasts (one horizon, enqueued between a batch filter's observations; the rest of the row: cssm_intervals.hip).
#include "cssm_internal.h"
#include "cssm_kernels.hip.h"
#include "cssm_posterior_move.hip.h"
#include "../../include/cssm_obs_draws.h"
#include "cssm_simulate_plan.h"

#include <cmath>

// (forecast_body<ROW>) what a block holds in LDS of its waves' extremes and PIT counts
template <int D>
struct FcRowShared {
  unsigned long long mm[CSSM_BLOCK / 64][D + 2][2];
  uint32_t pit[CSSM_BLOCK / 64][2];
};
template <int D>
__device__ __forceinline__ FcRowShared<D>& fc_row_shared() {
  __shared__ FcRowShared<D> s;
  return s;
}
// What the two forecasts share -- everything but where a particle starts and what moves it.  One thread per particle PAIR; a source
// `s` answers: begin (what it needs of the pair before the first load), x0 (component k of particle i, the pair's particle b, before
// the first chunk), step (one transition of the pair, or of its first particle alone) and obs (the observation parameters b draws with).
// ROW (k_forecast_row: a row of cssm_pf_filter_forecasts, enqueued between the observations of a batch filter): the one horizon of a
// forecast, and what the exact selection of cssm_intervals.hip starts from -- per block and row the smallest and the largest key
// (pmm), the block's two PIT counts against the record's datum (pit) --; the blocks clear the selection's histograms and counters, and
// a series on hold returns at once.  Geometry, keys and partial sums are the forecast's, so the means keep cssm_pf_forecast's bits.
struct FcRowOut {
  const Scalars* sc; unsigned long long* pmm /*[gridDim.x][D + 2][2]*/; uint32_t* pit /*[gridDim.x][2]*/; uint32_t* zero; size_t zero_words;
  unsigned long long* stamp; double y; int has_y;
};
__device__ __forceinline__ unsigned long long fc_shfl_xor(unsigned long long v, int off) {
  const uint32_t lo = __shfl_xor((uint32_t)v, off, 64), hi = __shfl_xor((uint32_t)(v >> 32), off, 64);
  return ((unsigned long long)hi << 32) | lo;
}
// (ROW) The wave's smallest and largest key of each of the D + 2 rows and its two PIT counts into LDS, a row at a time (nothing of it
// lives in registers across rows); threads without a particle are neutral.  All threads of the block call it.
template <int D>
__device__ __forceinline__ void fc_row_extremes(const FcRowOut* ro, bool live, bool hasb, const double (&xa)[D], const double (&xb)[D], double ea,
                                                double eb, double oa, double ob) {
  FcRowShared<D>& s = fc_row_shared<D>();
#pragma unroll
  for (int k = 0; k < D + 2; ++k) {
    const unsigned long long ka = cssm_order_key((k < D) ? xa[k % D] : (k == D ? ea : oa));
    const unsigned long long kb = cssm_order_key((k < D) ? xb[k % D] : (k == D ? eb : ob));
    unsigned long long mn = live ? ka : ~0ull, mx = live ? ka : 0ull;
    if (hasb) { mn = kb < mn ? kb : mn; mx = kb > mx ? kb : mx; }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const unsigned long long on = fc_shfl_xor(mn, off), ox = fc_shfl_xor(mx, off);
      mn = on < mn ? on : mn; mx = ox > mx ? ox : mx;
    }
    if ((threadIdx.x & 63) == 0) { s.mm[threadIdx.x >> 6][k][0] = mn; s.mm[threadIdx.x >> 6][k][1] = mx; }
  }
  const bool wy = ro->has_y != 0;
  uint32_t below = (uint32_t)(live && wy && oa < ro->y) + (uint32_t)(hasb && wy && ob < ro->y);
  uint32_t equal = (uint32_t)(live && wy && oa == ro->y) + (uint32_t)(hasb && wy && ob == ro->y);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) { below += __shfl_xor(below, off, 64); equal += __shfl_xor(equal, off, 64); }
  if ((threadIdx.x & 63) == 0) { s.pit[threadIdx.x >> 6][0] = below; s.pit[threadIdx.x >> 6][1] = equal; }
}
// ... and, behind the block's barrier, the block's own into memory
template <int D>
__device__ __forceinline__ void fc_row_store(const FcRowOut* ro) {
  FcRowShared<D>& s = fc_row_shared<D>();
  if (threadIdx.x < D + 2) {
    unsigned long long a = ~0ull, b = 0ull;
    for (int w = 0; w < CSSM_BLOCK / 64; ++w) {
      const unsigned long long oa = s.mm[w][threadIdx.x][0], ob = s.mm[w][threadIdx.x][1];
      a = oa < a ? oa : a; b = ob > b ? ob : b;
    }
    ro->pmm[((size_t)blockIdx.x * (D + 2) + threadIdx.x) * 2] = a;
    ro->pmm[((size_t)blockIdx.x * (D + 2) + threadIdx.x) * 2 + 1] = b;
  }
  if (threadIdx.x >= 64 && threadIdx.x < 66) {
    uint32_t c = 0;
    for (int w = 0; w < CSSM_BLOCK / 64; ++w) c += s.pit[w][threadIdx.x - 64];
    ro->pit[(size_t)blockIdx.x * 2 + (threadIdx.x - 64)] = c;
  }
}
template <int D, class Src, bool ROW = false>
__device__ __forceinline__ void forecast_body(Src& s, double* __restrict__ carry, int from_carry, int to_carry, uint64_t n,
                                              const StepRec* __restrict__ recs, uint32_t h0, uint32_t hc, const ModelK& mk, uint64_t key,
                                              const double* __restrict__ logtab, unsigned long long* __restrict__ keys,
                                              double* __restrict__ partial, double* __restrict__ samples, const FcRowOut* ro = nullptr) {
  constexpr int R = D + 2;   // rows per horizon: the D state components, eta, the observation
  __shared__ double s_p[CSSM_BLOCK / 64][R];
  if constexpr (ROW) {
    // (uniform: an earlier launch of the stream set it.  Bits 0 and 1 -- the weights of an earlier record were unusable: the call
    //  fails, its rows are unspecified, and nothing is drawn from a cloud nobody resampled)
    if (ro->sc->err & (IV_HELD | 3u)) return;
    if (blockIdx.x == 0 && threadIdx.x == 0) ro->stamp[0] = __builtin_amdgcn_s_memrealtime();
    for (size_t w = (size_t)blockIdx.x * CSSM_BLOCK + threadIdx.x; w < ro->zero_words; w += (size_t)gridDim.x * CSSM_BLOCK) ro->zero[w] = 0u;
  }
  const double* tab = stage_log_table(logtab);
  const uint64_t npairs = (n + 1) / 2;
  const uint64_t p = (uint64_t)blockIdx.x * CSSM_BLOCK + threadIdx.x;
  const bool live = p < npairs;
  const uint64_t ia = 2 * p, ib = ia + 1;
  const bool hasb = live && ib < n;
  const size_t rows = (size_t)hc * R;
  s.begin(live, hasb, ia, ib, key, from_carry);
  double xa[D], xb[D];
#pragma unroll
  for (int k = 0; k < D; ++k) {
    xa[k] = live ? (from_carry ? carry[(size_t)k * n + ia] : s.x0(0, ia, k)) : 0.0;
    xb[k] = hasb ? (from_carry ? carry[(size_t)k * n + ib] : s.x0(1, ib, k)) : 0.0;
  }
  for (uint32_t j = 0; j < hc; ++j) {
    const StepRec* rec = recs + j;
    const uint32_t h = h0 + j;
    double ga = 0.0, gb = 0.0, ea = 0.0, eb = 0.0, oa = 0.0, ob = 0.0;
    if (live) {
      s.step(hasb, mk, rec, key, ia, h, tab, xa, xb);
      ga = gamma_of<D>(mk, rec, xa);
      ea = link_of(mk.obs_kind, ga);
      cssm_obs_stream sa = cssm_obs_stream_at(key, ia, h);
      oa = cssm_obs_draw_one(&s.obs(0), ea, &sa, tab);
      unsigned long long* kr = keys + (size_t)j * R * n;
#pragma unroll
      for (int k = 0; k < D; ++k) kr[(size_t)k * n + ia] = cssm_order_key(xa[k]);
      kr[(size_t)D * n + ia] = cssm_order_key(ea);
      kr[(size_t)(D + 1) * n + ia] = cssm_order_key(oa);
      if (hasb) {
        gb = gamma_of<D>(mk, rec, xb);
        eb = link_of(mk.obs_kind, gb);
        cssm_obs_stream sb = cssm_obs_stream_at(key, ib, h);
        ob = cssm_obs_draw_one(&s.obs(1), eb, &sb, tab);
#pragma unroll
        for (int k = 0; k < D; ++k) kr[(size_t)k * n + ib] = cssm_order_key(xb[k]);
        kr[(size_t)D * n + ib] = cssm_order_key(eb);
        kr[(size_t)(D + 1) * n + ib] = cssm_order_key(ob);
      }
      if (samples) {   // rows of horizon j: state..., gamma, eta, obs
        double* sr = samples + (size_t)j * (D + 3) * n;
#pragma unroll
        for (int k = 0; k < D; ++k) sr[(size_t)k * n + ia] = xa[k];
        sr[(size_t)D * n + ia] = ga; sr[(size_t)(D + 1) * n + ia] = ea; sr[(size_t)(D + 2) * n + ia] = oa;
        if (hasb) {
#pragma unroll
          for (int k = 0; k < D; ++k) sr[(size_t)k * n + ib] = xb[k];
          sr[(size_t)D * n + ib] = gb; sr[(size_t)(D + 1) * n + ib] = eb; sr[(size_t)(D + 2) * n + ib] = ob;
        }
      }
    }
    // the block's partial sums of the horizon's R rows (threads without particles add zeros)
#pragma unroll
    for (int k = 0; k < R; ++k) {
      double v = (k < D) ? xa[k % D] + xb[k % D] : (k == D ? ea + eb : oa + ob);
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
      if ((threadIdx.x & 63) == 0) s_p[threadIdx.x >> 6][k] = v;
    }
    if constexpr (ROW) fc_row_extremes<D>(ro, live, hasb, xa, xb, ea, eb, oa, ob);
    __syncthreads();
    if (threadIdx.x < R) {
      double v = 0.0;
      for (int w = 0; w < CSSM_BLOCK / 64; ++w) v += s_p[w][threadIdx.x];
      partial[(size_t)blockIdx.x * rows + (size_t)j * R + threadIdx.x] = v;
    }
    if constexpr (ROW) fc_row_store<D>(ro);
    __syncthreads();
  }
  if (to_carry && live) {
#pragma unroll
    for (int k = 0; k < D; ++k) {
      carry[(size_t)k * n + ia] = xa[k];
      if (hasb) carry[(size_t)k * n + ib] = xb[k];
    }
  }
}

// Source 1: the handle's cloud under the handle's records.  A particle is gathered through the indirection k_summary_fill reads and
// moves by transition_one on the record (the unpaired last particle of an odd cloud: propagate_one); both particles draw with the
// model's one set of observation parameters.
template <int D>
struct CloudSrc {
  const double* __restrict__ src; size_t src_stride; const uint32_t* __restrict__ anc; const double* __restrict__ src2; size_t src2_stride;
  uint32_t n_split;
  cssm_obs_params op;
  __device__ __forceinline__ void begin(bool, bool, uint64_t, uint64_t, uint64_t, int) {}
  __device__ __forceinline__ double x0(int, uint64_t i, int k) const {
    const size_t j = anc ? (size_t)anc[i] : (size_t)i;
    return (src2 && j >= n_split)
        ? (src2_stride == 0 ? ld_sys_f64(src2 + (size_t)(j - n_split) * (size_t)(D + 1) + k) : ld_sys_f64(src2 + (size_t)k * src2_stride + (j - n_split)))
        : src[(size_t)k * src_stride + j];
  }
  __device__ __forceinline__ void step(bool hasb, const ModelK& mk, const StepRec* __restrict__ rec, uint64_t key, uint64_t ia, uint32_t h,
                                       const double* tab, double (&xa)[D], double (&xb)[D]) const {
    const double dt = rec->dt;
    if (hasb) pair_normals_feed<D>(key, ia, h, tab, [&](int b, int k, double e) { transition_one<D>(mk, rec, dt, k, b ? xb[k] : xa[k], e); });
    else propagate_one<D>(mk, rec, dt, key, ia, h, tab, xa);
  }
  __device__ __forceinline__ const cssm_obs_params& obs(int) const { return op; }
};

template <int D>
__global__ __launch_bounds__(CSSM_BLOCK) void k_forecast(const double* __restrict__ src, size_t src_stride, const uint32_t* __restrict__ anc,
                                                         const double* __restrict__ src2, size_t src2_stride, uint32_t n_split,
                                                         double* __restrict__ carry, int from_carry, int to_carry, uint64_t n,
                                                         const StepRec* __restrict__ recs, uint32_t h0, uint32_t hc, ModelK mk, uint64_t key,
                                                         cssm_obs_params op, const double* __restrict__ logtab,
                                                         unsigned long long* __restrict__ keys, double* __restrict__ partial,
                                                         double* __restrict__ samples) {
  CloudSrc<D> s{src, src_stride, anc, src2, src2_stride, n_split, op};
  forecast_body<D>(s, carry, from_carry, to_carry, n, recs, h0, hc, mk, key, logtab, keys, partial, samples);
}

// A row of cssm_pf_filter_forecasts: the single horizon `rec` from the cloud as it stands on the stream (forecast_body<ROW>).
template <int D>
__global__ __launch_bounds__(CSSM_BLOCK) void k_forecast_row(const double* __restrict__ src, size_t src_stride, const uint32_t* __restrict__ anc,
                                                             const double* __restrict__ src2, size_t src2_stride, uint32_t n_split, uint64_t n,
                                                             const StepRec* __restrict__ rec, ModelK mk, uint64_t key, cssm_obs_params op,
                                                             const double* __restrict__ logtab, unsigned long long* __restrict__ keys,
                                                             double* __restrict__ partial, FcRowOut ro) {
  CloudSrc<D> s{src, src_stride, anc, src2, src2_stride, n_split, op};
  forecast_body<D, CloudSrc<D>, true>(s, nullptr, 0, 0, n, rec, 0u, 1u, mk, key, logtab, keys, partial, nullptr, &ro);
}

// ---- forecasts from a joint posterior sample (cssm_pf_forecast_posterior): particle i starts from the state of pair pick_i and
// moves under that pair's parameter set.  A particle's set is the 3 D constrained values (mu, phi, sigma) of its posterior row, held in
// registers up to D = 8 and read from the row (L2-resident: M x (3 D + 1) doubles) above, where two particles' sets would spill
// (PostParams, cssm_posterior_move.hip.h).

// Source 2: a pair of the posterior sample per particle.  The first chunk gathers x0[pick_i] (M x D), every chunk loads row pick_i
// of `rows` (M x (3 D + 1): the parameter set, then the observation constant p0).  pick_i = pick[i], or the draw
// cssm_posterior_pick(key, i, M) when pick is null; pick_out (optional) receives it in the first chunk.  A component moves by
// transition_step on the coefficients cssm_sde_coef gives for the particle's own parameters (what cssm_build_rec puts into a record
// for them): the same arithmetic, so equal parameters give equal bits.  Philox streams and f are those of the handle's records.
template <int D>
struct PostSrc {
  static constexpr size_t S = 3 * D + 1;
  const double* __restrict__ x; const double* __restrict__ rows; uint64_t M; const uint32_t* __restrict__ pick; uint32_t* __restrict__ pick_out;
  cssm_obs_params opa, opb;   // (kind and df: the model's; p0: the particle's row)
  uint64_t ma, mb;
  PostParams<D> pa, pb;
  __device__ __forceinline__ void begin(bool live, bool hasb, uint64_t ia, uint64_t ib, uint64_t key, int from_carry) {
    auto pick_of = [&](uint64_t i) -> uint64_t { return pick ? (uint64_t)pick[i] : (uint64_t)cssm_posterior_pick(key, i, M); };
    ma = live ? pick_of(ia) : 0; mb = hasb ? pick_of(ib) : 0;
    if (pick_out && !from_carry) {
      if (live) pick_out[ia] = (uint32_t)ma;
      if (hasb) pick_out[ib] = (uint32_t)mb;
    }
    pa.load(rows + ma * S);
    pb.load(rows + mb * S);
    opa.p0 = rows[ma * S + 3 * D];
    opb.p0 = rows[mb * S + 3 * D];
  }
  __device__ __forceinline__ double x0(int b, uint64_t, int k) const { return x[(b ? mb : ma) * D + k]; }
  __device__ __forceinline__ void step(bool hasb, const ModelK& mk, const StepRec* __restrict__ rec, uint64_t key, uint64_t ia, uint32_t h,
                                       const double* tab, double (&xa)[D], double (&xb)[D]) const {
    post_step<D>(hasb, mk, rec->dt, key, ia, h, tab, pa, pb, xa, xb);
  }
  __device__ __forceinline__ const cssm_obs_params& obs(int b) const { return b ? opb : opa; }
};

template <int D>
__global__ __launch_bounds__(CSSM_BLOCK) void k_forecast_post(const double* __restrict__ x0, const double* __restrict__ rows, uint64_t M,
                                                              const uint32_t* __restrict__ pick, uint32_t* __restrict__ pick_out,
                                                              double* __restrict__ carry, int from_carry, int to_carry, uint64_t n,
                                                              const StepRec* __restrict__ recs, uint32_t h0, uint32_t hc, ModelK mk, uint64_t key,
                                                              int obs_df, const double* __restrict__ logtab,
                                                              unsigned long long* __restrict__ keys, double* __restrict__ partial,
                                                              double* __restrict__ samples) {
  PostSrc<D> s{x0, rows, M, pick, pick_out};
  s.opa.kind = s.opb.kind = mk.obs_kind; s.opa.df = s.opb.df = obs_df;
  forecast_body<D>(s, carry, from_carry, to_carry, n, recs, h0, hc, mk, key, logtab, keys, partial, samples);
}

// per row of the chunk: out[3 row] = mean (block partials / n), out[3 row + 1 / + 2] = the two selected order statistics
static __global__ __launch_bounds__(CSSM_BLOCK) void k_forecast_finish(const SelState* __restrict__ st, const double* __restrict__ partial, int nblocks,
                                                                       int rows, uint64_t n, double* __restrict__ out) {
  __shared__ double s_w[CSSM_BLOCK / 64];
  const int row = blockIdx.x;
  double v = 0.0;
  for (int b = threadIdx.x; b < nblocks; b += CSSM_BLOCK) v += partial[(size_t)b * rows + row];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
    for (int w = 0; w < CSSM_BLOCK / 64; ++w) s += s_w[w];
    out[3 * (size_t)row] = s / (double)n;
    out[3 * (size_t)row + 1] = cssm_order_unkey(st[row].prefix[0]);
    out[3 * (size_t)row + 2] = cssm_order_unkey(st[row].prefix[1]);
  }
}

static __global__ __launch_bounds__(CSSM_BLOCK) void k_obs_draw(cssm_obs_params op, const double* __restrict__ eta, uint64_t n, uint64_t key,
                                                                uint32_t step, const double* __restrict__ logtab, double* __restrict__ out) {
  const double* tab = stage_log_table(logtab);
  for (uint64_t i = (uint64_t)blockIdx.x * CSSM_BLOCK + threadIdx.x; i < n; i += (uint64_t)gridDim.x * CSSM_BLOCK) {
    cssm_obs_stream s = cssm_obs_stream_at(key, i, step);
    out[i] = cssm_obs_draw_one(&op, eta[i], &s, tab);
  }
}

// (the observation parameters of a draw, or the reference's exception as the message: cssm_obs_params_or_fail, cssm_model.cpp)
static int obs_params(int kind, int has_scale, double scale, int df, cssm_obs_params* op) { return cssm_obs_params_or_fail(kind, has_scale, scale, df, op); }

extern "C" int cssm_obs_draw(int obs_kind, const double* eta, size_t n, int has_scale, double scale, int df, uint64_t key, uint32_t step,
                             double* out, int device) {
  if (!eta || !out) return fail(CSSM_EINVAL_ARG, "null argument");
  if (n < 1) return fail(CSSM_EINVAL_ARG, "n must be at least 1");
  cssm_obs_params op;
  int rc = obs_params(obs_kind, has_scale, scale, df, &op);
  if (rc) return rc;
  rc = cssm_use_device(device);
  if (rc) return rc;
  CssmTemps tmp;
  double *de = nullptr, *dout = nullptr, *dtab = nullptr;
  HIP_ALLOC(tmp, de, n * 8); HIP_ALLOC(tmp, dout, n * 8); HIP_ALLOC(tmp, dtab, sizeof(CSSM_TAB));
  HIP_TRY(hipMemcpy(de, eta, n * 8, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(dtab, CSSM_TAB, sizeof(CSSM_TAB), hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_obs_draw, dim3(grid_for(n, CSSM_BLOCK, kGridCap)), dim3(CSSM_BLOCK), 0, 0, op, de, (uint64_t)n, key, step, dtab, dout);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(out, dout, n * 8, hipMemcpyDeviceToHost));
  return CSSM_OK;
}

// cssm_pf_filter_forecasts (cssm_intervals.hip): what cssm_pf_forecast refuses of the handle's model, in its words ...
int cssm_forecast_refuse_model(const cssm_pf* pf) {
  cssm_obs_params op;
  return obs_params(pf->obs_kind, pf->obs_has_scale, pf->obs_scale, pf->obs_df, &op);
}
// ... and the first launch of a row: the horizon of the device record `d_rec` under `key` from the cloud cssm_pf_forecast would read now
// (src / anc / src2 as the host holds them at this point of the enqueueing), one thread per particle pair
int cssm_forecast_row_launch(cssm_pf* pf, const StepRec* d_rec, uint64_t key, double y, int has_y, unsigned long long* keys, double* partial,
                             unsigned long long* pmm, uint32_t* pit, uint32_t* zero, size_t zero_words, unsigned long long* stamp, int nb_f) {
  cssm_obs_params op;
  int rc = obs_params(pf->obs_kind, pf->obs_has_scale, pf->obs_scale, pf->obs_df, &op);
  if (rc) return rc;
  const bool use_anc = pf->anc_valid;
  const FcRowOut ro{pf->sc, pmm, pit, zero, zero_words, stamp, y, has_y};
  DISPATCH_D(pf->d, hipLaunchKernelGGL(k_forecast_row<D>, dim3(nb_f), dim3(CSSM_BLOCK), 0, pf->stream, pf->src, pf->src_stride,
                                       (const uint32_t*)(use_anc ? pf->anc : nullptr), use_anc ? pf->src2 : nullptr, pf->src2_stride, pf->n_split,
                                       (uint64_t)pf->n, d_rec, pf->mk, key, op, (const double*)pf->d_logtab, keys, partial, ro));
  HIP_TRY(hipGetLastError());
  return CSSM_OK;
}

// (horizon times after t_start, finite and non-decreasing: cssm_check_times, cssm_model.cpp)
static int check_times(const double* t, size_t H, double t_start, const char* start) { return cssm_check_times(t, H, t_start, start); }

// The chunked driver of both forecasts.  Per chunk of horizons [h0, h0 + hn): launch(h0, hn, recs of the chunk, carry, from_carry,
// to_carry, keys, partial, samples, blocks) runs the forecast kernel (nb_f blocks, one thread per particle pair), then one radix
// selection over the chunk's rows and k_forecast_finish; the results land in the outputs, the device times in pf->forecast_ms.
template <class Launch>
static int forecast_chunks(cssm_pf* pf, double t_start, const double* t, size_t H, double interval, double* state_mean, double* state_lower,
                           double* state_upper, double* eta_mean, double* eta_lower, double* eta_upper, double* obs_mean, double* obs_lower,
                           double* obs_upper, double* samples, Launch&& launch) {
  HIP_TRY(hipSetDevice(pf->device));
  const int d = pf->d, R = d + 2;
  const uint64_t n = pf->n;
  // horizons per chunk: the order keys of a chunk (R rows of n keys per horizon) within the cap; grid.y of the selection <= 65535
  const size_t cap = pf->forecast_cap ? pf->forecast_cap : ((size_t)1 << 30);
  size_t hc = cap / ((size_t)R * n * 8);
  hc = std::max<size_t>(1, std::min<size_t>({hc, H, (size_t)(65535 / R)}));
  const size_t rows_max = hc * (size_t)R;
  const uint64_t npairs = (n + 1) / 2;
  const int nb_f = (int)((npairs + CSSM_BLOCK - 1) / CSSM_BLOCK);
  const int nb_s = grid_for(n, CSSM_BLOCK, 1024);
  std::vector<StepRec> hrec(H);
  for (size_t h = 0; h < H; ++h) cssm_build_rec(pf, h ? t[h - 1] : t_start, t[h], 0.0, 0, (uint32_t)h, &hrec[h]);
  std::vector<SelState> hst(rows_max);
  std::vector<double> hout(3 * rows_max);
  CssmTemps tmp;
  StepRec* drec = nullptr; double* carry = nullptr; unsigned long long* keys = nullptr; double* partial = nullptr; SelState* st = nullptr;
  uint32_t* hist = nullptr; double* out = nullptr; double* dsamp = nullptr;
  hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
  double ms_kernel = 0.0, ms_select = 0.0;
  const bool chunked = hc < H;
  HIP_ALLOC(tmp, drec, H * sizeof(StepRec));
  HIP_ALLOC(tmp, keys, rows_max * n * 8);
  HIP_ALLOC(tmp, partial, (size_t)nb_f * rows_max * 8);
  HIP_ALLOC(tmp, st, rows_max * sizeof(SelState));
  HIP_ALLOC(tmp, hist, rows_max * 512 * 4);
  HIP_ALLOC(tmp, out, 3 * rows_max * 8);
  if (chunked) HIP_ALLOC(tmp, carry, (size_t)d * n * 8);
  if (samples) HIP_ALLOC(tmp, dsamp, hc * (size_t)(d + 3) * n * 8);
  for (int i = 0; i < 3; ++i) HIP_TRY(tmp.event(ev[i]));
  HIP_TRY(hipMemcpyAsync(drec, hrec.data(), H * sizeof(StepRec), hipMemcpyHostToDevice, pf->stream));
  for (size_t h0 = 0; h0 < H; h0 += hc) {
    const size_t hn = std::min(hc, H - h0), rows = hn * (size_t)R;
    for (size_t r = 0; r < rows; ++r) sel_ranks(hst[r], n, interval, (int)(r % R) < d);
    HIP_TRY(hipMemcpyAsync(st, hst.data(), rows * sizeof(SelState), hipMemcpyHostToDevice, pf->stream));
    HIP_TRY(hipMemsetAsync(hist, 0, rows * 512 * 4, pf->stream));
    HIP_TRY(hipEventRecord(ev[0], pf->stream));
    launch(h0, hn, (const StepRec*)(drec + h0), carry, (int)(h0 > 0), (int)(chunked && h0 + hn < H), keys, partial, dsamp, nb_f);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(ev[1], pf->stream));
    for (int shift = 56; shift >= 0; shift -= 8) {
      hipLaunchKernelGGL(k_sel_hist, dim3(nb_s, (unsigned)rows), dim3(CSSM_BLOCK), 0, pf->stream, (const unsigned long long*)keys, (size_t)n, n,
                         (const SelState*)st, shift, hist);
      hipLaunchKernelGGL(k_sel_pick, dim3((unsigned)rows), dim3(2), 0, pf->stream, st, shift, hist);
    }
    hipLaunchKernelGGL(k_forecast_finish, dim3((unsigned)rows), dim3(CSSM_BLOCK), 0, pf->stream, (const SelState*)st, (const double*)partial, nb_f,
                       (int)rows, n, out);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(ev[2], pf->stream));
    HIP_TRY(hipMemcpyAsync(hout.data(), out, 3 * rows * 8, hipMemcpyDeviceToHost, pf->stream));
    if (samples) HIP_TRY(hipMemcpyAsync(samples + h0 * (size_t)(d + 3) * n, dsamp, hn * (size_t)(d + 3) * n * 8, hipMemcpyDeviceToHost, pf->stream));
    HIP_TRY(hipStreamSynchronize(pf->stream));
    {
      float a = 0.f, b = 0.f;
      HIP_TRY(hipEventElapsedTime(&a, ev[0], ev[1]));
      HIP_TRY(hipEventElapsedTime(&b, ev[1], ev[2]));
      ms_kernel += a; ms_select += b;
    }
    for (size_t j = 0; j < hn; ++j) {
      const size_t h = h0 + j;
      const double* o = hout.data() + 3 * j * (size_t)R;
      for (int k = 0; k < d; ++k) {
        if (state_mean) state_mean[h * d + k] = o[3 * k];
        if (state_lower) state_lower[h * d + k] = o[3 * k + 1];
        if (state_upper) state_upper[h * d + k] = o[3 * k + 2];
      }
      if (eta_mean) eta_mean[h] = o[3 * d];
      if (eta_lower) eta_lower[h] = o[3 * d + 1];
      if (eta_upper) eta_upper[h] = o[3 * d + 2];
      if (obs_mean) obs_mean[h] = o[3 * (d + 1)];
      if (obs_lower) obs_lower[h] = o[3 * (d + 1) + 1];
      if (obs_upper) obs_upper[h] = o[3 * (d + 1) + 2];
    }
  }
  pf->forecast_ms[0] = ms_kernel;
  pf->forecast_ms[1] = ms_select;
  return CSSM_OK;
}

extern "C" int cssm_pf_forecast(cssm_pf* pf, const double* t, size_t H, uint64_t key, double interval, double* state_mean, double* state_lower,
                                double* state_upper, double* eta_mean, double* eta_lower, double* eta_upper, double* obs_mean, double* obs_lower,
                                double* obs_upper, double* samples) {
  if (!pf) return fail(CSSM_EINVAL_ARG, "null handle");
  if (pf->sharded) return fail(CSSM_ESTATE, "forecasts of a sharded filter are not supported: forecast from a single-GPU handle");
  if (!pf->initialised) return fail(CSSM_ESTATE, "not initialised");
  if (!(interval > 0.0 && interval <= 1.0)) return fail(CSSM_EINVAL_ARG, "interval must be in (0, 1]");
  if (H == 0) return CSSM_OK;
  if (!t) return fail(CSSM_EINVAL_ARG, "null argument");
  if (H > 0xffffffffull) return fail(CSSM_EINVAL_ARG, "too many horizons");
  cssm_obs_params op;
  int rc = obs_params(pf->obs_kind, pf->obs_has_scale, pf->obs_scale, pf->obs_df, &op);
  if (rc) return rc;
  rc = check_times(t, H, pf->t, "the cloud's time");
  if (rc) return rc;
  const uint64_t n = pf->n;
  return forecast_chunks(pf, pf->t, t, H, interval, state_mean, state_lower, state_upper, eta_mean, eta_lower, eta_upper, obs_mean, obs_lower,
                         obs_upper, samples,
                         [&](size_t h0, size_t hn, const StepRec* recs, double* carry, int from_carry, int to_carry, unsigned long long* keys,
                             double* partial, double* dsamp, int nb_f) {
                           const bool use_anc = !from_carry && pf->anc_valid;
                           DISPATCH_D(pf->d, hipLaunchKernelGGL(k_forecast<D>, dim3(nb_f), dim3(CSSM_BLOCK), 0, pf->stream, pf->src, pf->src_stride,
                                                                (const uint32_t*)(use_anc ? pf->anc : nullptr), use_anc ? pf->src2 : nullptr,
                                                                pf->src2_stride, pf->n_split, carry, from_carry, to_carry, n, recs, (uint32_t)h0,
                                                                (uint32_t)hn, pf->mk, key, op, (const double*)pf->d_logtab, keys, partial, dsamp));
                         });
}

extern "C" int cssm_pf_forecast_posterior(cssm_pf* pf, const cssm_model_desc* desc, const double* theta, size_t n_theta, const double* x, size_t M,
                                          double t0, const double* t, size_t H, const uint32_t* pick, uint64_t key, double interval,
                                          double* state_mean, double* state_lower, double* state_upper, double* eta_mean, double* eta_lower,
                                          double* eta_upper, double* obs_mean, double* obs_lower, double* obs_upper, double* samples,
                                          uint32_t* pick_out) {
  if (!pf) return fail(CSSM_EINVAL_ARG, "null handle");
  if (pf->sharded) return fail(CSSM_ESTATE, "forecasts of a sharded filter are not supported: forecast from a single-GPU handle");
  if (!desc || !theta || !x) return fail(CSSM_EINVAL_ARG, "null argument");
  if (M == 0) return fail(CSSM_EINVAL_ARG, "the posterior sample is empty (M = 0)");
  if (M > 0xffffffffull) return fail(CSSM_EINVAL_ARG, "the posterior sample has more than 2^32 - 1 rows");
  if (!(interval > 0.0 && interval <= 1.0)) return fail(CSSM_EINVAL_ARG, "interval must be in (0, 1]");
  if (!std::isfinite(t0)) return fail(CSSM_EINVAL_ARG, "t0 is not finite");
  if (H && !t) return fail(CSSM_EINVAL_ARG, "null argument");
  if (H > 0xffffffffull) return fail(CSSM_EINVAL_ARG, "too many horizons");
  if (!desc->leaves || desc->n_leaves < 1) return fail(CSSM_EINVAL_DESC, "null model descriptor");
  cssm_obs_params op;   // (the model's observation: LGCP has none; each row's constant goes into `rows`)
  int rc = obs_params(pf->obs_kind, desc->leaves[0].has_scale, desc->leaves[0].scale, pf->obs_df, &op);
  if (rc) return rc;
  std::vector<double> rows;
  rc = cssm_posterior_rows(pf, desc, theta, n_theta, M, rows);
  if (rc) return rc;
  const int d = pf->d;
  for (size_t m = 0; m < M; ++m)
    for (int k = 0; k < d; ++k)
      if (!std::isfinite(x[m * d + k])) return fail(CSSM_EINVAL_ARG, "x row %zu: component %d is not finite", m, k);
  const uint64_t n = pf->n;
  if (pick)
    for (uint64_t i = 0; i < n; ++i)
      if (pick[i] >= M) return fail(CSSM_EINVAL_ARG, "pick[%llu] = %u is not below M = %zu", (unsigned long long)i, pick[i], M);
  rc = check_times(t, H, t0, "t0 =");
  if (rc) return rc;
  if (H == 0) {   // nothing to forecast: the picks alone
    if (pick_out) for (uint64_t i = 0; i < n; ++i) pick_out[i] = pick ? pick[i] : cssm_posterior_pick(key, i, M);
    return CSSM_OK;
  }
  HIP_TRY(hipSetDevice(pf->device));
  CssmTemps tmp;
  double *dx = nullptr, *drows = nullptr;
  uint32_t *dpick = nullptr, *dpick_out = nullptr;
  HIP_ALLOC(tmp, dx, M * (size_t)d * 8);
  HIP_ALLOC(tmp, drows, rows.size() * 8);
  if (pick) HIP_ALLOC(tmp, dpick, n * 4);
  if (pick_out) HIP_ALLOC(tmp, dpick_out, n * 4);
  HIP_TRY(hipMemcpy(dx, x, M * (size_t)d * 8, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(drows, rows.data(), rows.size() * 8, hipMemcpyHostToDevice));
  if (pick) HIP_TRY(hipMemcpy(dpick, pick, n * 4, hipMemcpyHostToDevice));
  rc = forecast_chunks(pf, t0, t, H, interval, state_mean, state_lower, state_upper, eta_mean, eta_lower, eta_upper, obs_mean, obs_lower,
                       obs_upper, samples,
                       [&](size_t h0, size_t hn, const StepRec* recs, double* carry, int from_carry, int to_carry, unsigned long long* keys,
                           double* partial, double* dsamp, int nb_f) {
                         DISPATCH_D(d, hipLaunchKernelGGL(k_forecast_post<D>, dim3(nb_f), dim3(CSSM_BLOCK), 0, pf->stream, (const double*)dx,
                                                          (const double*)drows, (uint64_t)M, (const uint32_t*)dpick, dpick_out, carry, from_carry,
                                                          to_carry, n, recs, (uint32_t)h0, (uint32_t)hn, pf->mk, key, pf->obs_df,
                                                          (const double*)pf->d_logtab, keys, partial, dsamp));
                       });
  if (!rc && pick_out) HIP_TRY(hipMemcpy(pick_out, dpick_out, n * 4, hipMemcpyDeviceToHost));
  return rc;
}

extern "C" int cssm_pf_forecast_last_ms(cssm_pf* pf, double* ms2) {
  if (!pf || !ms2) return fail(CSSM_EINVAL_ARG, "null argument");
  if (pf->forecast_ms[0] < 0.0) return fail(CSSM_ESTATE, "no forecast has run on this handle");
  ms2[0] = pf->forecast_ms[0];
  ms2[1] = pf->forecast_ms[1];
  return CSSM_OK;
}

extern "C" uint64_t cssm_pf_observation_index(const cssm_pf* pf) { return pf ? pf->step : 0; }
