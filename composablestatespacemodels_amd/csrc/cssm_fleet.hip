// cssm_fleet.hip -- host side of the fleet filter (include/cssm_pf.h, "fleet of independent series"): S series of one model structure,
// N <= CSSM_FLEET_MAX_N particles each, parameters / Philox key / data / clock of its own per series, advanced by ONE launch whose
// blocks are the series (cssm_fleet.hip.h: k_fleet_series, one object per latent dimension).  Also k_fleet_summary (getIntervals of
// every series, one block per (series, row)).  A fleet call never degenerates into S single-handle runs: what the kernels do not
// serve is refused when the fleet is created or parameterised.
//
// Per-observation constants: the host builds every record with cssm_build_rec -- the function the single handle uses, so its bits by
// construction -- and uploads the compact form (FleetRecHead + 5 d doubles: 80 + 40 d bytes per observation, not sizeof(StepRec)).
// Records of different series are independent: large calls build them on a few host threads.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <thread>

#include "cssm_internal.h"
#include "cssm_kernels.hip.h"
#include "cssm_fleet.hip.h"
#include "cssm_fleet_forecast.hip.h"
#include "cssm_fleet_interp.hip.h"

static_assert(CSSM_FLEET_MAX_N <= 4096, "k_fleet_summary sorts at most 4096 keys in LDS; k_fleet_series holds 12 bytes per particle there");

struct cssm_fleet {
  int device = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   // filter / step call, summary, forecast,
                                                                                                 // [6], [7]: a path launch's upload | kernel | read-back
  uint32_t n = 0, S = 0;
  int d = 0, threads = 64;
  size_t lds = 0;
  HostModel base;                       // the structure every series shares
  std::vector<HostModel> models;        // per series: parameters, key (HostModel::seed), n_global = n
  std::vector<double> t;                // per series: its clock
  std::vector<uint32_t> step;           // ... its observation index (Philox counter word; parity = the buffer that holds its cloud)
  std::vector<uint8_t> live;            // ... a cloud exists (initialised and not failed since)
  std::vector<int> obs_has_scale;       // ... the leftmost leaf's scale as stored (forecasts: cssm_obs_params_make)
  std::vector<double> obs_scale;
  bool par_dirty = true;
  // device
  double* state = nullptr; uint32_t* anc = nullptr; FleetSeries* ser = nullptr; FleetPar* par = nullptr; double* logtab = nullptr;
  unsigned char* d_stage = nullptr; size_t stage_cap = 0;
  double* d_ll_t = nullptr; int32_t* d_ess_t = nullptr; size_t res_cap = 0;
  double* d_tmp = nullptr;              // d x n: cssm_fleet_get_particles
  unsigned char* d_fcr = nullptr; size_t fcr_cap = 0;   // cssm_fleet_filter_forecasts / _step_forecast, grow-only: rows of [d + 2][3] doubles, then rows of 2 PIT counts
  double* d_iv = nullptr; size_t iv_cap = 0;       // cssm_fleet_filter_intervals / _step_intervals, grow-only: rows of [d + 1][3] (mean, lower, upper)
  double* d_path = nullptr; size_t path_cap = 0;   // cssm_fleet_filter, grow-only: [S][d] last rows, then (asked for) the R + S rows of the paths
  float ms_upload = -1.f, ms_kernel = -1.f;        // ... of its last launch
  double ms_build = 0.0;                           // ... host time of its records
  double pm_split[6] = {0, 0, 0, 0, 0, 0};         // cssm_fleet_pmmh_run: see cssm_fleet_pmmh_last_split
  double* d_sm = nullptr; size_t sm_cap = 0;   // summary: [S][d] f coefficients, [S][d + 1][3] results, [S] buffer numbers
  // host staging (pinned)
  unsigned char* h_stage = nullptr; size_t h_stage_cap = 0;
  std::vector<FleetSeries> h_ser;
  float ms_call = -1.f, ms_summary = -1.f, ms_forecast = -1.f;
  // forecasts (cssm_fleet_forecast), grow-only: [off | keys | obs params | buffer numbers | records | results] and its pinned mirror,
  // eta / obs staging of every series, the samples of one chunk of series (at most fc_samp_max bytes: CSSM_OPT_FORECAST_CAP)
  unsigned char* d_fc = nullptr; size_t fc_cap = 0;
  unsigned char* h_fc = nullptr; size_t h_fc_cap = 0;
  double* d_fc_stage = nullptr;
  double* d_fc_samp = nullptr; size_t fc_samp_cap = 0;
  size_t fc_samp_max = (size_t)1 << 30;
  int fc_select = 0;                    // CSSM_OPT_FLEET_SELECT: 0 = by N (CSSM_FLEET_SELECT_MIN_N), 1 = bitonic sort, 2 = radix select
  // interpolation (cssm_fleet_interpolate), grow-only: one chunk's [off | records | f coefficients | series scalars | results] and its
  // pinned mirror; one chunk's lineage history (clouds, then ancestors: at most ip_hist_max bytes, CSSM_OPT_INTERP_CAP)
  unsigned char* d_ip = nullptr; size_t ip_cap = 0;
  unsigned char* h_ip = nullptr; size_t h_ip_cap = 0;
  unsigned char* d_ip_hist = nullptr; size_t ip_hist_cap = 0;
  size_t ip_hist_max = (size_t)1 << 30;
  hipEvent_t ev_ip[3] = {nullptr, nullptr, nullptr};   // before the forward launch | between the two | behind the lineage launch
  double ms_ip[2] = {-1.0, -1.0};                      // ... of the last interpolation, summed over its chunks
  bool ip_ran = false;
};

#define FLEET_SERVED "cssm_pf_* (one handle per series) and cssm_pfb_* (batch of chains) serve it"

template <class F>
static void fleet_parallel(size_t count, size_t work, F f) {
  unsigned nt = std::thread::hardware_concurrency();
  nt = std::min<unsigned>(nt ? nt : 1u, 8u);
  if (work < 8192 || count < 2 * nt || nt < 2) { f((size_t)0, count); return; }
  std::vector<std::thread> th;
  const size_t per = (count + nt - 1) / nt;
  for (unsigned q = 0; q < nt; ++q) {
    const size_t lo = std::min(count, q * per), hi = std::min(count, lo + per);
    if (lo < hi) th.emplace_back([=] { f(lo, hi); });
  }
  for (auto& x : th) x.join();
}

static void fleet_pack_rec(const HostModel& m, double t_prev, double t, double y, int has, uint32_t step, unsigned char* dst, uint32_t* pick = nullptr) {
  StepRec r;
  cssm_build_rec(&m, t_prev, t, y, has, step, &r);
  if (pick) *pick = r.pick;
  FleetRecHead h;
  h.y = r.y; h.c[0] = r.c[0]; h.c[1] = r.c[1]; h.c[2] = r.c[2]; h.c[3] = r.c[3]; h.cdf = r.cdf; h.u = r.u; h.dt = r.dt; h.ref = r.ref;
  h.has_obs = r.has_obs; h.step = r.step;
  memcpy(dst, &h, sizeof h);
  double* tail = reinterpret_cast<double*>(dst + sizeof h);
  for (int k = 0; k < m.d; ++k) for (int q = 0; q < 4; ++q) tail[4 * k + q] = r.coef[k][q];
  for (int k = 0; k < m.d; ++k) tail[4 * m.d + k] = r.fco[k];
}

// getIntervals of every series (model/ParticleFilter.scala:415-424), one block per (series, row); rows 0 .. D-1 the state components,
// row D eta = link(f(x, t)).  The row's N values are sorted in LDS as order-preserving keys (bitonic network over the next power of
// two, padded with the largest key): the order statistics are exact.  The mean is a plain fp64 sum / N.
template <int D>
__global__ __launch_bounds__(CSSM_BLOCK) void k_fleet_summary(const double* __restrict__ state, const uint32_t* __restrict__ anc,
                                                              const uint32_t* __restrict__ cur, const double* __restrict__ fco, uint32_t n,
                                                              uint32_t np2, ModelK mk, uint32_t lo_state, uint32_t hi_state,
                                                              uint32_t lo_eta, uint32_t hi_eta, double* __restrict__ out) {
  extern __shared__ unsigned long long s_keys[];
  __shared__ double s_p[CSSM_BLOCK / 64];
  const uint32_t k = blockIdx.x, row = blockIdx.y, tid = threadIdx.x;
  double* o = out + ((size_t)k * (D + 1) + row) * 3u;
  const uint32_t c = cur[k];
  if (c > 1u) {                                                 // (uniform) no cloud: not initialised, or failed since
    if (tid < 3u) o[tid] = cssm_nan();
    return;
  }
  const double* src = state + ((size_t)k * 2u + c) * D * n;
  const uint32_t* ga = anc + (size_t)k * n;
  double acc = 0.0;
  for (uint32_t i = tid; i < np2; i += CSSM_BLOCK) {
    unsigned long long key = ~0ull;
    if (i < n) {
      const uint32_t j = ga[i];
      double v;
      if (row < (uint32_t)D) {
        v = src[(size_t)row * n + j];
      } else {
        double x[D];
#pragma unroll
        for (int q = 0; q < D; ++q) x[q] = src[(size_t)q * n + j];
        v = link_of(mk.obs_kind, gamma_coef<D>(mk, fco + (size_t)k * D, x));
      }
      acc += v;
      key = cssm_order_key(v);
    }
    s_keys[i] = key;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
  if ((tid & 63u) == 0u) s_p[tid >> 6] = acc;
  for (uint32_t k2 = 2u; k2 <= np2; k2 <<= 1) {
    for (uint32_t j = k2 >> 1; j > 0u; j >>= 1) {
      __syncthreads();
      for (uint32_t i = tid; i < np2; i += CSSM_BLOCK) {
        const uint32_t p = i ^ j;
        if (p > i) {
          const unsigned long long x = s_keys[i], y = s_keys[p];
          const bool up = (i & k2) == 0u;
          if ((x > y) == up) { s_keys[i] = y; s_keys[p] = x; }
        }
      }
    }
  }
  __syncthreads();
  if (tid == 0) {
    double s = 0.0;
    for (int w = 0; w < CSSM_BLOCK / 64; ++w) s += s_p[w];
    o[0] = s / (double)n;
    o[1] = cssm_order_unkey(s_keys[row < (uint32_t)D ? lo_state : lo_eta]);
    o[2] = cssm_order_unkey(s_keys[row < (uint32_t)D ? hi_state : hi_eta]);
  }
}

extern "C" void cssm_fleet_destroy(cssm_fleet* f) {
  if (!f) return;
  (void)hipSetDevice(f->device);
  if (f->stream) (void)hipStreamSynchronize(f->stream);
  void* ptrs[] = {f->state, f->anc, f->ser, f->par, f->logtab, f->d_stage, f->d_ll_t, f->d_ess_t, f->d_tmp, f->d_path, f->d_iv, f->d_fcr, f->d_sm, f->d_fc, f->d_fc_stage, f->d_fc_samp, f->d_ip, f->d_ip_hist};
  for (void* p : ptrs) if (p) (void)hipFree(p);
  if (f->h_stage) (void)hipHostFree(f->h_stage);
  if (f->h_fc) (void)hipHostFree(f->h_fc);
  if (f->h_ip) (void)hipHostFree(f->h_ip);
  for (hipEvent_t e : f->ev) if (e) (void)hipEventDestroy(e);
  for (hipEvent_t e : f->ev_ip) if (e) (void)hipEventDestroy(e);
  if (f->stream) (void)hipStreamDestroy(f->stream);
  delete f;
}

extern "C" int cssm_fleet_create(const cssm_model_desc* desc, uint64_t n_particles, uint32_t n_series, int device, cssm_fleet** out) {
  if (!out) return fail(CSSM_EINVAL_ARG, "out is null");
  *out = nullptr;
  if (n_particles < 1 || n_particles > CSSM_FLEET_MAX_N)
    return fail(CSSM_EINVAL_ARG, "a fleet holds 1 .. %d particles per series (a cloud lives in one workgroup's LDS), not %llu; " FLEET_SERVED,
                CSSM_FLEET_MAX_N, (unsigned long long)n_particles);
  if (n_series < 1) return fail(CSSM_EINVAL_ARG, "a fleet needs at least one series");
  HostModel base;
  int rc = cssm_build_model(&base, desc, false);
  if (rc) return rc;
  if (base.obs_kind == CSSM_OBS_LGCP)
    return fail(CSSM_EINVAL_DESC, "the fleet filter does not serve the LGCP observation model (sub-stepped events); " FLEET_SERVED);
  rc = cssm_use_device(device);
  if (rc) return rc;
  cssm_fleet* f = new cssm_fleet();
  f->device = device; f->n = (uint32_t)n_particles; f->S = n_series; f->d = base.d;
  base.n_global = n_particles; base.seed = 0;
  f->base = base;
  const uint32_t S = n_series, n = f->n;
  f->models.assign(S, base);
  f->t.assign(S, 0.0); f->step.assign(S, 0u); f->live.assign(S, 0); f->h_ser.resize(S);
  f->obs_has_scale.assign(S, desc->leaves[0].has_scale); f->obs_scale.assign(S, desc->leaves[0].scale);
  // block size: about four particles per thread, whole waves, at most CSSM_FLEET_MAX_THREADS (results do not depend on it)
  f->threads = (int)std::min<uint32_t>(CSSM_FLEET_MAX_THREADS, std::max<uint32_t>(64u, ((n + 3u) / 4u + 63u) & ~63u));
  f->lds = (size_t)((n + 1u) & ~1u) * 8u + (size_t)n * 4u;
  auto bail = [&](int code, const char* what) { cssm_fleet_destroy(f); return fail(code, "fleet of %u series x %u particles: %s", S, n, what); };
  if (hipStreamCreateWithFlags(&f->stream, hipStreamNonBlocking) != hipSuccess) return bail(CSSM_EHIP, "hipStreamCreate");
  for (hipEvent_t& e : f->ev) if (hipEventCreate(&e) != hipSuccess) return bail(CSSM_EHIP, "hipEventCreate");
  for (hipEvent_t& e : f->ev_ip) if (hipEventCreate(&e) != hipSuccess) return bail(CSSM_EHIP, "hipEventCreate");
  const size_t rows = (size_t)S * 2u * f->d * n;
  if (hipMalloc(&f->state, rows * 8) != hipSuccess || hipMalloc(&f->anc, (size_t)S * n * 4) != hipSuccess ||
      hipMalloc(&f->ser, (size_t)S * sizeof(FleetSeries)) != hipSuccess || hipMalloc(&f->par, (size_t)S * sizeof(FleetPar)) != hipSuccess ||
      hipMalloc(&f->logtab, sizeof(CSSM_TAB)) != hipSuccess || hipMalloc(&f->d_tmp, (size_t)f->d * n * 8) != hipSuccess)
    return bail(CSSM_ENOMEM, "device memory (16 d N bytes of state per series)");
  if (hipMemcpyAsync(f->logtab, CSSM_TAB, sizeof(CSSM_TAB), hipMemcpyHostToDevice, f->stream) != hipSuccess ||
      hipMemsetAsync(f->ser, 0, (size_t)S * sizeof(FleetSeries), f->stream) != hipSuccess ||
      hipStreamSynchronize(f->stream) != hipSuccess)
    return bail(CSSM_EHIP, "uploading the contract's table");
  *out = f;
  return CSSM_OK;
}

extern "C" uint32_t cssm_fleet_num_series(const cssm_fleet* f) { return f ? f->S : 0u; }
extern "C" uint64_t cssm_fleet_num_particles(const cssm_fleet* f) { return f ? f->n : 0u; }

extern "C" int cssm_fleet_set_option(cssm_fleet* f, int option, int value) {
  if (!f) return fail(CSSM_EINVAL_ARG, "null fleet");
  if (option == CSSM_OPT_FORECAST_CAP) {   // KiB of samples one chunk of series holds on the device; 0 = 1 GiB
    if (value < 0) return fail(CSSM_EINVAL_ARG, "CSSM_OPT_FORECAST_CAP must not be negative (got %d)", value);
    f->fc_samp_max = value ? (size_t)value << 10 : (size_t)1 << 30;
    return CSSM_OK;
  }
  if (option == CSSM_OPT_INTERP_CAP) {   // KiB of lineage history one chunk of series holds on the device; 0 = 1 GiB
    if (value < 0) return fail(CSSM_EINVAL_ARG, "CSSM_OPT_INTERP_CAP must not be negative (got %d)", value);
    f->ip_hist_max = value ? (size_t)value << 10 : (size_t)1 << 30;
    return CSSM_OK;
  }
  if (option == CSSM_OPT_FLEET_SELECT) {
    if (value < 0 || value > 2) return fail(CSSM_EINVAL_ARG, "CSSM_OPT_FLEET_SELECT is 0 (by N), 1 (sort) or 2 (radix select), not %d", value);
    f->fc_select = value;
    return CSSM_OK;
  }
  if (option != CSSM_OPT_RESAMPLER) return fail(CSSM_EINVAL_ARG, "a fleet has no option %d", option);
  if (value != CSSM_RESAMPLE_SYSTEMATIC)
    return fail(CSSM_EINVAL_ARG, "the fleet filter resamples systematically only (resampler %d asked for); " FLEET_SERVED, value);
  return CSSM_OK;
}

extern "C" int cssm_fleet_set_params(cssm_fleet* f, const cssm_model_desc* const* descs) {
  if (!f || !descs) return fail(CSSM_EINVAL_ARG, "null argument");
  // all or nothing: a descriptor of another structure leaves the fleet as it was
  std::vector<HostModel> next(f->S);
  const cssm_model_desc* last = nullptr;
  for (uint32_t k = 0; k < f->S; ++k) {
    if (k > 0 && descs[k] == last) { next[k] = next[k - 1]; continue; }     // (pointers may repeat)
    next[k] = f->base;
    const int rc = cssm_build_model(&next[k], descs[k], true);
    if (rc) { const std::string keep = cssm_last_error(); return fail(rc, "series %u: %s", k, keep.c_str()); }
    last = descs[k];
  }
  for (uint32_t k = 0; k < f->S; ++k) {
    next[k].seed = f->models[k].seed; next[k].n_global = f->n;
    f->obs_has_scale[k] = descs[k]->leaves[0].has_scale; f->obs_scale[k] = descs[k]->leaves[0].scale;
  }
  f->models.swap(next);
  f->par_dirty = true;
  return CSSM_OK;
}

extern "C" int cssm_fleet_reseed(cssm_fleet* f, const uint64_t* seeds) {
  if (!f || !seeds) return fail(CSSM_EINVAL_ARG, "null argument");
  for (uint32_t k = 0; k < f->S; ++k) f->models[k].seed = seeds[k];
  f->par_dirty = true;
  return CSSM_OK;
}

static int fleet_upload_par(cssm_fleet* f) {
  if (!f->par_dirty) return CSSM_OK;
  std::vector<FleetPar> hp(f->S);
  for (uint32_t k = 0; k < f->S; ++k) {
    const HostModel& m = f->models[k];
    memset(&hp[k], 0, sizeof(FleetPar));
    hp[k].seed = m.seed;
    for (int c = 0; c < m.d; ++c) { hp[k].m0[c] = m.comp[c].m0; hp[k].sd0[c] = std::sqrt(m.comp[c].c0); }
  }
  HIP_TRY(hipMemcpyAsync(f->par, hp.data(), (size_t)f->S * sizeof(FleetPar), hipMemcpyHostToDevice, f->stream));
  HIP_TRY(hipStreamSynchronize(f->stream));   // (hp is pageable and dies here)
  f->par_dirty = false;
  return CSSM_OK;
}

// staging layout of a launch: [S + 1 offsets (u64)] [S control words (u32), padded to 8 bytes] [R compact records]
static size_t fleet_stage_head(const cssm_fleet* f) { return ((size_t)f->S + 1u) * 8u + (((size_t)f->S * 4u + 7u) & ~(size_t)7u); }

// What a launch that also writes getIntervals of its clouds carries and brings back (k_fleet_series<D, false, false, true>).
struct FleetIv {
  double interval;
  bool step;                  // one row per series (cssm_fleet_step_intervals), not T_k + 1 rows per series
  size_t rows = 0;            // of [d + 1][3] doubles: S, or R + S
  std::vector<double> out;    // the rows as the device left them; NaN where no block wrote
};

// What a launch that also forecasts every record before it is stepped carries and brings back (k_fleet_series<D, false, false, false, true>).
struct FleetFc {
  double interval;
  const uint64_t* keys;       // the caller's, one per record of the call as the caller counts them ([off[S]], or [S] for a step), or null
  bool step = false;          // one row per series (cssm_fleet_step_forecast), not one per record
  size_t rows = 0;            // of [d + 2][3] doubles and of 2 counts: S, or R
  std::vector<double> out;    // the rows as the device left them; NaN where no block wrote
  std::vector<int32_t> pit;   // ... -1 where no block wrote
  std::vector<int> fc_rc;     // [S]: the forecast's own status of every series
  std::string scale_msg;      // the reference's exception for the first series without the scale its observation needs
};
// behind the R records of such a launch: [R keys (u64)] [R data (f64)] [S observation parameters] [R flags (u32)]
static_assert(sizeof(cssm_obs_params) == 16, "the [S] array of observation parameters is uploaded as it is");
static size_t fleet_fc_bytes(const cssm_fleet* f, size_t R) { return R * 16u + (size_t)f->S * sizeof(cssm_obs_params) + ((R * 4u + 7u) & ~(size_t)7u); }

// (picks: the launch also carries R sampleOne slots, uint32 each, behind the records; iv: S x d f coefficients, F at every series' t0;
// fc: fleet_fc_bytes -- a launch carries one of the three at most)
static int fleet_ensure(cssm_fleet* f, size_t R, bool picks = false, bool iv = false, bool fc = false) {
  const size_t need = fleet_stage_head(f) + R * CSSM_FLEET_REC_BYTES(f->d) + (picks ? R * 4u : 0u) + (iv ? (size_t)f->S * f->d * 8u : 0u) +
                      (fc ? fleet_fc_bytes(f, R) : 0u);
  if (need > f->h_stage_cap) {
    if (f->h_stage) (void)hipHostFree(f->h_stage);
    f->h_stage = nullptr; f->h_stage_cap = 0;
    if (hipHostMalloc((void**)&f->h_stage, need + need / 4, hipHostMallocDefault) != hipSuccess) return fail(CSSM_ENOMEM, "fleet: %zu bytes of pinned staging", need);
    f->h_stage_cap = need + need / 4;
  }
  if (need > f->stage_cap) {
    if (f->d_stage) (void)hipFree(f->d_stage);
    f->d_stage = nullptr; f->stage_cap = 0;
    if (hipMalloc(&f->d_stage, need + need / 4) != hipSuccess) return fail(CSSM_ENOMEM, "fleet: %zu bytes of records", need);
    f->stage_cap = need + need / 4;
  }
  const size_t rr = std::max<size_t>(R, 1);
  if (rr > f->res_cap) {
    if (f->d_ll_t) (void)hipFree(f->d_ll_t);
    if (f->d_ess_t) (void)hipFree(f->d_ess_t);
    f->d_ll_t = nullptr; f->d_ess_t = nullptr; f->res_cap = 0;
    if (hipMalloc(&f->d_ll_t, (rr + rr / 4) * 8) != hipSuccess || hipMalloc(&f->d_ess_t, (rr + rr / 4) * 4) != hipSuccess)
      return fail(CSSM_ENOMEM, "fleet: per-observation results");
    f->res_cap = rr + rr / 4;
  }
  return CSSM_OK;
}

// k_fleet_series of the fleet's latent dimension (one object per dimension: cssm_fleet_d.hip)
static int fleet_series_launch(int d, const FleetLaunch& l) {
  int hrc = 0;
  switch (d) {
#define FLEET_CASE(D) case D: hrc = cssm_fleet_launch_d##D(l); break;
    FLEET_CASE(1) FLEET_CASE(2) FLEET_CASE(3) FLEET_CASE(4) FLEET_CASE(5) FLEET_CASE(6) FLEET_CASE(7) FLEET_CASE(8)
    FLEET_CASE(9) FLEET_CASE(10) FLEET_CASE(11) FLEET_CASE(12) FLEET_CASE(13) FLEET_CASE(14) FLEET_CASE(15) FLEET_CASE(16)
#undef FLEET_CASE
    default: return fail(CSSM_EINVAL_DESC, "latent dimension %d", d);
  }
  if (hrc) return fail(CSSM_EHIP, "k_fleet_series: %s", hipGetErrorString((hipError_t)hrc));
  return CSSM_OK;
}

// upload the staged launch, run it, bring the series' scalars (and, asked for, the per-observation results) back; synchronises.
// want_path: the staged launch carries its picks and runs k_fleet_series<D, true>; path_out (may be null) / last_out receive the rows.
// iv: the staged launch carries the f coefficients of every series' t0 behind its records and runs k_fleet_series<D, false, false, true>.
// fc: the staged launch carries fleet_fc_bytes behind its records and runs k_fleet_series<D, false, false, false, true>.
static int fleet_launch(cssm_fleet* f, size_t R, double* ll_t, int32_t* ess_t, bool want_path = false, double* path_out = nullptr, double* last_out = nullptr,
                        FleetIv* iv = nullptr, FleetFc* fc = nullptr) {
  int rc = fleet_upload_par(f);
  if (rc) return rc;
  const size_t head = fleet_stage_head(f), recs = R * CSSM_FLEET_REC_BYTES(f->d),
               bytes = head + recs + (want_path ? R * 4u : 0u) + (iv ? (size_t)f->S * f->d * 8u : 0u) + (fc ? fleet_fc_bytes(f, R) : 0u);
  const size_t n_fco = fc ? fc->rows * (size_t)(f->d + 2) * 3u : 0u, n_fcr = n_fco * 8u + (fc ? fc->rows * 8u : 0u);   // (bytes: doubles, then counts)
  if (n_fcr > f->fcr_cap) {
    if (f->d_fcr) (void)hipFree(f->d_fcr);
    f->d_fcr = nullptr; f->fcr_cap = 0;
    if (hipMalloc(&f->d_fcr, n_fcr + n_fcr / 4) != hipSuccess) return fail(CSSM_ENOMEM, "fleet: %zu bytes of one-step-ahead forecasts", n_fcr);
    f->fcr_cap = n_fcr + n_fcr / 4;
  }
  if (fc && !f->d_fc_stage && hipMalloc(&f->d_fc_stage, (size_t)f->S * 2u * f->n * 8u) != hipSuccess) {
    f->d_fc_stage = nullptr;
    return fail(CSSM_ENOMEM, "fleet forecast: 16 N bytes of staging per series");
  }
  const size_t n_iv = iv ? iv->rows * (size_t)(f->d + 1) * 3u : 0u;
  if (n_iv > f->iv_cap) {
    if (f->d_iv) (void)hipFree(f->d_iv);
    f->d_iv = nullptr; f->iv_cap = 0;
    if (hipMalloc(&f->d_iv, (n_iv + n_iv / 4) * 8) != hipSuccess) return fail(CSSM_ENOMEM, "fleet: %zu bytes of filtered intervals", n_iv * 8);
    f->iv_cap = n_iv + n_iv / 4;
  }
  const size_t n_last = (size_t)f->S * f->d, n_rows = n_last + (path_out ? (R + f->S) * (size_t)f->d : 0u);
  if (want_path && n_rows > f->path_cap) {
    if (f->d_path) (void)hipFree(f->d_path);
    f->d_path = nullptr; f->path_cap = 0;
    if (hipMalloc(&f->d_path, (n_rows + n_rows / 4) * 8) != hipSuccess) return fail(CSSM_ENOMEM, "fleet: %zu bytes of sampled paths", n_rows * 8);
    f->path_cap = n_rows + n_rows / 4;
  }
  HIP_TRY(hipEventRecord(f->ev[0], f->stream));
  HIP_TRY(hipMemcpyAsync(f->d_stage, f->h_stage, bytes, hipMemcpyHostToDevice, f->stream));
  if (R) {   // records a failed series never reaches read as NaN / -1
    HIP_TRY(hipMemsetAsync(f->d_ll_t, 0xff, R * 8, f->stream));
    HIP_TRY(hipMemsetAsync(f->d_ess_t, 0xff, R * 4, f->stream));
  }
  if (want_path) {   // ... and the rows it never records as NaN
    HIP_TRY(hipMemsetAsync(f->d_path, 0xff, n_rows * 8, f->stream));
    HIP_TRY(hipEventRecord(f->ev[6], f->stream));
  }
  if (iv) HIP_TRY(hipMemsetAsync(f->d_iv, 0xff, n_iv * 8, f->stream));   // ... and the rows it never summarises
  if (n_fcr) HIP_TRY(hipMemsetAsync(f->d_fcr, 0xff, n_fcr, f->stream));  // ... or never forecasts (NaN; -1 in the counts)
  FleetLaunch l;
  l.args.n = f->n; l.args.state = f->state; l.args.anc = f->anc; l.args.ser = f->ser; l.args.par = f->par;
  l.args.off = reinterpret_cast<const unsigned long long*>(f->d_stage);
  l.args.ctl = reinterpret_cast<const uint32_t*>(f->d_stage + ((size_t)f->S + 1u) * 8u);
  l.args.recs = f->d_stage + head;
  l.args.ll_t = f->d_ll_t; l.args.ess_t = f->d_ess_t; l.args.logtab = f->logtab; l.args.mk = f->base.mk;
  l.args.picks = want_path ? reinterpret_cast<const uint32_t*>(f->d_stage + head + recs) : nullptr;
  l.args.path = (want_path && path_out) ? f->d_path + n_last : nullptr;
  l.args.last = want_path ? f->d_path : nullptr;
  l.args.hist = nullptr; l.args.hanc = nullptr; l.args.hser = nullptr; l.args.k0 = 0u;
  l.args.iv_fco0 = nullptr; l.args.iv_out = nullptr; l.args.iv_rows = 0u; l.args.iv_np2 = 0u; l.args.iv_rk = FleetRowRanks{0u, 0u, 0u, 0u};
  l.args.fc = FleetOneStep{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  l.n_series = f->S; l.path = want_path; l.threads = f->threads; l.lds = f->lds; l.stream = f->stream;
  if (fc) {
    SelState rs, re;   // the ranks of a state row and of the eta / obs rows, as cssm_fleet_forecast takes them
    sel_ranks(rs, f->n, fc->interval, true);
    sel_ranks(re, f->n, fc->interval, false);
    uint32_t np2 = 2u;
    while (np2 < f->n) np2 <<= 1;
    const unsigned char* x = f->d_stage + head + recs;
    l.args.fc.keys = reinterpret_cast<const unsigned long long*>(x);
    l.args.fc.y = reinterpret_cast<const double*>(x + R * 8u);
    l.args.fc.op = reinterpret_cast<const cssm_obs_params*>(x + R * 16u);
    l.args.fc.flags = reinterpret_cast<const uint32_t*>(x + R * 16u + (size_t)f->S * sizeof(cssm_obs_params));
    l.args.fc.stage = f->d_fc_stage;
    l.args.fc.out = reinterpret_cast<double*>(f->d_fcr);
    l.args.fc.pit = reinterpret_cast<int32_t*>(f->d_fcr + n_fco * 8u);
    l.args.iv_rows = fc->step ? 1u : 0u; l.args.iv_np2 = np2;
    l.args.iv_rk = FleetRowRanks{(uint32_t)rs.rank[0], (uint32_t)rs.rank[1], (uint32_t)re.rank[0], (uint32_t)re.rank[1]};
    l.fcst = true; l.lds = (size_t)np2 * 8u + (size_t)f->n * 4u;   // the keys of a row's sort take the weights' place
    fc->out.resize(n_fco); fc->pit.resize(fc->rows * 2u);
  }
  if (iv) {
    SelState rs, re;   // the ranks of a state row and of the eta row, as cssm_fleet_summary takes them
    sel_ranks(rs, f->n, iv->interval, true);
    sel_ranks(re, f->n, iv->interval, false);
    uint32_t np2 = 2u;
    while (np2 < f->n) np2 <<= 1;
    l.args.iv_fco0 = reinterpret_cast<const double*>(f->d_stage + head + recs);
    l.args.iv_out = f->d_iv; l.args.iv_rows = iv->step ? 1u : 0u; l.args.iv_np2 = np2;
    l.args.iv_rk = FleetRowRanks{(uint32_t)rs.rank[0], (uint32_t)rs.rank[1], (uint32_t)re.rank[0], (uint32_t)re.rank[1]};
    l.ival = true; l.lds = (size_t)np2 * 8u + (size_t)f->n * 4u;   // the keys of a row's sort take the weights' place
    iv->out.resize(n_iv);
  }
  rc = fleet_series_launch(f->d, l);
  if (rc) return rc;
  if (want_path) HIP_TRY(hipEventRecord(f->ev[7], f->stream));
  HIP_TRY(hipMemcpyAsync(f->h_ser.data(), f->ser, (size_t)f->S * sizeof(FleetSeries), hipMemcpyDeviceToHost, f->stream));
  if (want_path && path_out) HIP_TRY(hipMemcpyAsync(path_out, f->d_path + n_last, (n_rows - n_last) * 8, hipMemcpyDeviceToHost, f->stream));
  if (want_path && last_out) HIP_TRY(hipMemcpyAsync(last_out, f->d_path, n_last * 8, hipMemcpyDeviceToHost, f->stream));
  if (R && ll_t) HIP_TRY(hipMemcpyAsync(ll_t, f->d_ll_t, R * 8, hipMemcpyDeviceToHost, f->stream));
  if (R && ess_t) HIP_TRY(hipMemcpyAsync(ess_t, f->d_ess_t, R * 4, hipMemcpyDeviceToHost, f->stream));
  if (n_iv) HIP_TRY(hipMemcpyAsync(iv->out.data(), f->d_iv, n_iv * 8, hipMemcpyDeviceToHost, f->stream));
  if (n_fcr) {
    HIP_TRY(hipMemcpyAsync(fc->out.data(), f->d_fcr, n_fco * 8u, hipMemcpyDeviceToHost, f->stream));
    HIP_TRY(hipMemcpyAsync(fc->pit.data(), f->d_fcr + n_fco * 8u, fc->rows * 8u, hipMemcpyDeviceToHost, f->stream));
  }
  HIP_TRY(hipEventRecord(f->ev[1], f->stream));
  HIP_TRY(hipStreamSynchronize(f->stream));
  if (hipEventElapsedTime(&f->ms_call, f->ev[0], f->ev[1]) != hipSuccess) f->ms_call = -1.f;
  if (want_path) {
    if (hipEventElapsedTime(&f->ms_upload, f->ev[0], f->ev[6]) != hipSuccess) f->ms_upload = -1.f;
    if (hipEventElapsedTime(&f->ms_kernel, f->ev[6], f->ev[7]) != hipSuccess) f->ms_kernel = -1.f;
  }
  return CSSM_OK;
}

// the staged arrays of a FleetFc launch of R records (fleet_fc_bytes) in the pinned staging
struct FleetFcStage {
  unsigned long long* keys; double* y; cssm_obs_params* op; uint32_t* flags;
};
static FleetFcStage fleet_fc_stage(const cssm_fleet* f, size_t R) {
  unsigned char* x = f->h_stage + fleet_stage_head(f) + R * CSSM_FLEET_REC_BYTES(f->d);
  return FleetFcStage{reinterpret_cast<unsigned long long*>(x), reinterpret_cast<double*>(x + R * 8u), reinterpret_cast<cssm_obs_params*>(x + R * 16u),
                      reinterpret_cast<uint32_t*>(x + R * 16u + (size_t)f->S * sizeof(cssm_obs_params))};
}
// the observation parameters of series k's draws and the forecast's own status of the series (runs: the call has a record for it)
static void fleet_fc_series(const cssm_fleet* f, uint32_t k, bool runs, FleetFc* fc, cssm_obs_params* op) {
  memset(op, 0, sizeof *op);
  fc->fc_rc[k] = CSSM_OK;
  if (!runs) return;
  if (cssm_obs_params_or_fail(f->base.obs_kind, f->obs_has_scale[k], f->obs_scale[k], f->base.obs_df, op)) {
    if (fc->scale_msg.empty()) fc->scale_msg = "series " + std::to_string(k) + ": " + cssm_last_error();
    fc->fc_rc[k] = CSSM_EINVAL_ARG;
  }
}
// One row of a FleetFc launch into the caller's arrays; a row without a forecast (ok == false) reads NaN and -1
struct FleetFcOut {
  double *state_mean, *state_lower, *state_upper, *eta_mean, *eta_lower, *eta_upper, *obs_mean, *obs_lower, *obs_upper;
  int32_t *obs_below, *obs_equal;
};
static void fleet_fc_row(const cssm_fleet* f, const FleetFc& fc, size_t src_row, bool ok, const FleetFcOut& o, size_t row) {
  const int d = f->d;
  const double* v = fc.out.data() + src_row * (size_t)(d + 2) * 3u;
  auto at = [&](int r, int q) { return ok ? v[3 * r + q] : cssm_nan(); };
  for (int c = 0; c < d; ++c) {
    if (o.state_mean) o.state_mean[row * d + c] = at(c, 0);
    if (o.state_lower) o.state_lower[row * d + c] = at(c, 1);
    if (o.state_upper) o.state_upper[row * d + c] = at(c, 2);
  }
  if (o.eta_mean) o.eta_mean[row] = at(d, 0);
  if (o.eta_lower) o.eta_lower[row] = at(d, 1);
  if (o.eta_upper) o.eta_upper[row] = at(d, 2);
  if (o.obs_mean) o.obs_mean[row] = at(d + 1, 0);
  if (o.obs_lower) o.obs_lower[row] = at(d + 1, 1);
  if (o.obs_upper) o.obs_upper[row] = at(d + 1, 2);
  if (o.obs_below) o.obs_below[row] = ok ? fc.pit[2 * src_row] : -1;
  if (o.obs_equal) o.obs_equal[row] = ok ? fc.pit[2 * src_row + 1] : -1;
}

// llFilter / filter of every series: the records of all of them built (threaded above 8192), ONE upload, ONE launch, ONE read-back.
// want_path: `filter` -- the sampleOne slots travel behind the records, path_out (may be null) and last_out (may be null) are written.
static int fleet_filter_all(cssm_fleet* f, const uint64_t* off, const double* t, const double* y, const uint8_t* has_obs, double* ll_out, double* ll_t,
                            int32_t* ess_t, bool want_path, double* path_out, double* last_out, int* rc_out, FleetIv* iv = nullptr, FleetFc* fc = nullptr) {
  const uint32_t S = f->S;
  if (off[0] != 0) return fail(CSSM_EINVAL_ARG, "off[0] must be 0");
  for (uint32_t k = 0; k < S; ++k)
    if (off[k + 1] < off[k]) return fail(CSSM_EINVAL_ARG, "off must be non-decreasing (off[%u] = %llu > off[%u] = %llu)", k, (unsigned long long)off[k],
                                         k + 1, (unsigned long long)off[k + 1]);
  const size_t R = (size_t)off[S];
  if (R && (!t || !y)) return fail(CSSM_EINVAL_ARG, "null data");
  HIP_TRY(hipSetDevice(f->device));
  const auto tb0 = std::chrono::steady_clock::now();
  int rc = fleet_ensure(f, R, want_path, iv != nullptr, fc != nullptr);
  if (rc) return rc;
  unsigned long long* h_off = reinterpret_cast<unsigned long long*>(f->h_stage);
  uint32_t* h_ctl = reinterpret_cast<uint32_t*>(f->h_stage + ((size_t)S + 1u) * 8u);
  unsigned char* h_recs = f->h_stage + fleet_stage_head(f);
  const size_t RB = CSSM_FLEET_REC_BYTES(f->d);
  FleetFcStage fs{nullptr, nullptr, nullptr, nullptr};
  if (fc) {                                                              // (the reference's exception is one message: formed in order)
    fs = fleet_fc_stage(f, R);
    fc->fc_rc.assign(S, CSSM_OK);
    for (uint32_t k = 0; k < S; ++k) fleet_fc_series(f, k, off[k + 1] > off[k], fc, &fs.op[k]);
    if (R & 1u) fs.flags[R] = 0u;                                        // (the padding travels too)
  }
  uint32_t* h_picks = want_path ? reinterpret_cast<uint32_t*>(h_recs + R * RB) : nullptr;
  double* h_fco0 = iv ? reinterpret_cast<double*>(h_recs + R * RB) : nullptr;   // (a launch carries picks or these, never both)
  for (uint32_t k = 0; k <= S; ++k) h_off[k] = off[k];
  std::vector<double> t0(S, 0.0);
  fleet_parallel(S, R, [&](size_t lo, size_t hi) {
    for (size_t k = lo; k < hi; ++k) {
      const size_t a = (size_t)off[k], b = (size_t)off[k + 1];
      h_ctl[k] = (b > a) ? CSSM_FLEET_CTL_INIT : 0u;
      if (h_fco0) for (int c = 0; c < f->d; ++c) h_fco0[k * f->d + c] = 0.0;
      if (b == a) continue;
      double m = t[a];
      for (size_t s = a + 1; s < b; ++s) m = (t[s] < m) ? t[s] : m;      // data.minBy(_.t).t
      t0[k] = m;
      if (h_fco0) {                                                      // F(t0): t0 need not be the first record's time
        StepRec r0;
        cssm_build_rec(&f->models[k], m, m, 0.0, 0, 0u, &r0);
        for (int c = 0; c < f->d; ++c) h_fco0[k * f->d + c] = r0.fco[c];
      }
      double tp = m;
      for (size_t s = a; s < b; ++s) {
        fleet_pack_rec(f->models[k], tp, t[s], y[s], has_obs ? (int)has_obs[s] : 1, (uint32_t)(s - a), h_recs + s * RB, h_picks ? h_picks + s : nullptr);
        if (fc) {   // the forecast of record s: cssm_fleet_forecast's own refusals of a time, the key, the datum as given
          const bool on = fc->fc_rc[k] == CSSM_OK && std::isfinite(t[s]) && t[s] >= tp;
          fs.flags[s] = on ? (CSSM_FLEET_FC_ON | ((has_obs ? has_obs[s] : 1) ? CSSM_FLEET_FC_HAS : 0u)) : 0u;
          fs.keys[s] = fc->keys ? fc->keys[s] : cssm_pf_run_key(f->models[k].seed, (1ull << 63) | (uint64_t)(s - a));
          fs.y[s] = y[s];
        }
        tp = t[s];
      }
    }
  });
  if (want_path) f->ms_build = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tb0).count();
  if (iv) { iv->step = false; iv->rows = R + S; }
  if (fc) { fc->step = false; fc->rows = R; }
  rc = fleet_launch(f, R, ll_t, ess_t, want_path, path_out, last_out, iv, fc);
  if (rc) return rc;
  for (uint32_t k = 0; k < S; ++k) {
    const size_t a = (size_t)off[k], b = (size_t)off[k + 1];
    if (b == a) { rc_out[k] = CSSM_EINVAL_ARG; ll_out[k] = cssm_nan(); continue; }   // (the reference's minBy throws on an empty Vector)
    const FleetSeries& s = f->h_ser[k];
    if (s.err) {
      rc_out[k] = CSSM_ENONFINITE; ll_out[k] = cssm_nan(); f->live[k] = 0;
    } else {
      rc_out[k] = CSSM_OK; ll_out[k] = s.ll; f->live[k] = 1; f->t[k] = t[b - 1]; f->step[k] = (uint32_t)(b - a);
    }
  }
  return CSSM_OK;
}

extern "C" int cssm_fleet_ll_filter(cssm_fleet* f, const uint64_t* off, const double* t, const double* y, const uint8_t* has_obs,
                                    double* ll_out, double* ll_t, int32_t* ess_t, int* rc_out) {
  if (!f || !off || !ll_out || !rc_out) return fail(CSSM_EINVAL_ARG, "null argument");
  return fleet_filter_all(f, off, t, y, has_obs, ll_out, ll_t, ess_t, false, nullptr, nullptr, rc_out);
}

// filter (model/ParticleFilter.scala:152-158) of every series: cssm_fleet_ll_filter, and one particle of the initial cloud and of the
// cloud after every record (Resampling.sampleOne).  What needs no fleet is refused first, so that it is refused on any host.
extern "C" int cssm_fleet_filter(cssm_fleet* f, const uint64_t* off, const double* t, const double* y, const uint8_t* has_obs, double* ll_out,
                                 double* ll_t, int32_t* ess_t, double* path_out, double* last_out, int* rc_out) {
  if (!off) return fail(CSSM_EINVAL_ARG, "off is null");
  if (!ll_out || !rc_out) return fail(CSSM_EINVAL_ARG, "ll_out / rc_out is null");
  if (!path_out && !last_out)
    return fail(CSSM_EINVAL_ARG, "neither path_out nor last_out is given: cssm_fleet_ll_filter is the call that records no path");
  if (off[0] != 0) return fail(CSSM_EINVAL_ARG, "off[0] must be 0");
  if (!t || !y) return fail(CSSM_EINVAL_ARG, "null data");
  if (!f) return fail(CSSM_EINVAL_ARG, "null fleet");
  return fleet_filter_all(f, off, t, y, has_obs, ll_out, ll_t, ess_t, true, path_out, last_out, rc_out);
}

// One row of a FleetIv launch into the caller's arrays: the d state rows and the eta row as the block left them, eta of the mean formed
// here as cssm_fleet_summary forms it (:420) from the row's own f coefficients.
struct FleetIvOut {
  double *state_mean, *state_lower, *state_upper, *eta_of_mean, *eta_lower, *eta_upper;
};
static void fleet_iv_row(const cssm_fleet* f, uint32_t k, const double* src, const double* fco, const FleetIvOut& o, size_t row) {
  const int d = f->d;
  double mean[CSSM_MAX_DIM];
  for (int c = 0; c < d; ++c) {
    mean[c] = src[c * 3];
    if (o.state_mean) o.state_mean[row * d + c] = src[c * 3];
    if (o.state_lower) o.state_lower[row * d + c] = src[c * 3 + 1];
    if (o.state_upper) o.state_upper[row * d + c] = src[c * 3 + 2];
  }
  if (o.eta_lower) o.eta_lower[row] = src[d * 3 + 1];
  if (o.eta_upper) o.eta_upper[row] = src[d * 3 + 2];
  if (o.eta_of_mean) o.eta_of_mean[row] = cssm_eta_of_mean(f->models[k], fco, mean);
}

// examples/Filtering.scala:24-31 of every series: cssm_fleet_ll_filter, and getIntervals (model/ParticleFilter.scala:415-424) of the initial
// cloud and of the cloud after every record, written by the series' own workgroup inside the one launch.  What needs no fleet is refused
// first, so that it is refused on any host.
extern "C" int cssm_fleet_filter_intervals(cssm_fleet* f, const uint64_t* off, const double* t, const double* y, const uint8_t* has_obs, double interval,
                                           double* ll_out, double* ll_t, int32_t* ess_t, double* state_mean, double* state_lower, double* state_upper,
                                           double* eta_of_mean, double* eta_lower, double* eta_upper, int* rc_out) {
  if (!off) return fail(CSSM_EINVAL_ARG, "off is null");
  if (!ll_out || !rc_out) return fail(CSSM_EINVAL_ARG, "ll_out / rc_out is null");
  if (off[0] != 0) return fail(CSSM_EINVAL_ARG, "off[0] must be 0");
  if (!t || !y) return fail(CSSM_EINVAL_ARG, "null data");
  if (!(interval > 0.0 && interval <= 1.0)) return fail(CSSM_EINVAL_ARG, "interval must be in (0, 1]");
  if (!f) return fail(CSSM_EINVAL_ARG, "null fleet");
  FleetIv iv;
  iv.interval = interval;
  int rc = fleet_filter_all(f, off, t, y, has_obs, ll_out, ll_t, ess_t, false, nullptr, nullptr, rc_out, &iv);
  if (rc) return rc;
  const uint32_t S = f->S;
  const int d = f->d;
  const size_t R = (size_t)off[S], RB = CSSM_FLEET_REC_BYTES(d), rowsz = (size_t)(d + 1) * 3u;
  const FleetIvOut o{state_mean, state_lower, state_upper, eta_of_mean, eta_lower, eta_upper};
  for (double* p : {state_mean, state_lower, state_upper}) if (p) std::fill(p, p + (R + S) * (size_t)d, cssm_nan());
  for (double* p : {eta_of_mean, eta_lower, eta_upper}) if (p) std::fill(p, p + (R + S), cssm_nan());
  const unsigned char* h_recs = f->h_stage + fleet_stage_head(f);   // (the staged launch is still there: the records' f coefficients)
  const double* h_fco0 = reinterpret_cast<const double*>(h_recs + R * RB);
  fleet_parallel(S, R, [&](size_t lo, size_t hi) {
    for (size_t k = lo; k < hi; ++k) {
      const size_t a = (size_t)off[k], b = (size_t)off[k + 1];
      if (b == a) continue;                                         // no records: NaN in its single row
      const FleetSeries& s = f->h_ser[k];
      const size_t nrows = s.err ? (size_t)s.fail_rec + 1u : b - a + 1u;   // a failure at observation s keeps rows 0 .. s
      for (size_t i = 0; i < nrows; ++i) {
        const double* fco = i ? reinterpret_cast<const double*>(h_recs + (a + i - 1) * RB + sizeof(FleetRecHead)) + 4 * d : h_fco0 + k * d;
        fleet_iv_row(f, (uint32_t)k, iv.out.data() + (a + k + i) * rowsz, fco, o, a + k + i);
      }
    }
  });
  return CSSM_OK;
}

// ParticleFilter.getMeanForecast mapped over the filter stream (model/ParticleFilter.scala:368-409) of every series: cssm_fleet_ll_filter,
// and before every record is stepped the forecast of its time from the cloud before it -- cssm_fleet_forecast with that single horizon --
// by the series' own workgroup inside the ONE launch.  What needs no fleet is refused first, so that it is refused on any host.
extern "C" int cssm_fleet_filter_forecasts(cssm_fleet* f, const uint64_t* off, const double* t, const double* y, const uint8_t* has_obs,
                                           const uint64_t* keys, double interval, double* ll_out, double* ll_t, int32_t* ess_t, double* state_mean,
                                           double* state_lower, double* state_upper, double* eta_mean, double* eta_lower, double* eta_upper,
                                           double* obs_mean, double* obs_lower, double* obs_upper, int32_t* obs_below, int32_t* obs_equal,
                                           int* rc_out, int* fc_rc_out) {
  if (!off) return fail(CSSM_EINVAL_ARG, "off is null");
  if (!ll_out || !rc_out || !fc_rc_out) return fail(CSSM_EINVAL_ARG, "ll_out / rc_out / fc_rc_out is null");
  if (off[0] != 0) return fail(CSSM_EINVAL_ARG, "off[0] must be 0");
  if (!t || !y) return fail(CSSM_EINVAL_ARG, "null data");
  if (!(interval > 0.0 && interval <= 1.0)) return fail(CSSM_EINVAL_ARG, "interval must be in (0, 1]");
  if (!f) return fail(CSSM_EINVAL_ARG, "null fleet");
  FleetFc fc;
  fc.interval = interval; fc.keys = keys;
  int rc = fleet_filter_all(f, off, t, y, has_obs, ll_out, ll_t, ess_t, false, nullptr, nullptr, rc_out, nullptr, &fc);
  if (rc) return rc;
  const uint32_t S = f->S;
  const size_t R = (size_t)off[S];
  const FleetFcOut o{state_mean, state_lower, state_upper, eta_mean, eta_lower, eta_upper, obs_mean, obs_lower, obs_upper, obs_below, obs_equal};
  const FleetFcStage fs = fleet_fc_stage(f, R);                         // (the staged launch is still there: the records' flags)
  fleet_parallel(S, R, [&](size_t lo, size_t hi) {
    for (size_t k = lo; k < hi; ++k) {
      const size_t a = (size_t)off[k], b = (size_t)off[k + 1];
      fc_rc_out[k] = fc.fc_rc[k];
      const FleetSeries& s = f->h_ser[k];
      const size_t nrows = (b > a && s.err) ? (size_t)s.fail_rec + 1u : b - a;   // a failure at observation s keeps rows 0 .. s
      for (size_t i = 0; i < b - a; ++i) fleet_fc_row(f, fc, a + i, i < nrows && (fs.flags[a + i] & CSSM_FLEET_FC_ON), o, a + i);
    }
  });
  if (!fc.scale_msg.empty()) (void)fail(CSSM_EINVAL_ARG, "%s", fc.scale_msg.c_str());   // (the call succeeds; the message names the first such series)
  return CSSM_OK;
}

// ParticleMetropolisHastings (model/PMMH.scala:68-81,114-123) for S chains in lockstep, a chain per series: chain k is cssm_pmmh_run
// with theta0[k], seeds[k] and series k's slice of the data -- proposals, filter keys and decisions are cssm_pmmh_chain_*'s, as in
// every PMMH driver -- and an iteration's S filters are ONE fleet launch that brings back S x d doubles of sampled states.
#define FLEET_PMMH_SERVED "cssm_pmmh_run_batched (a batch of chains, each spread over the GPU) serves it"
extern "C" int cssm_fleet_pmmh_run(cssm_fleet* f, const cssm_model_desc* desc, const double* theta0, size_t n_theta, double delta, const uint64_t* off,
                                   const double* t, const double* y, const uint8_t* has_obs, const uint64_t* seeds, size_t n_iters, double* ll,
                                   double* theta, int32_t* accepted, double* last_state) {
  if (!desc || !theta0 || !off || !t || !y || !seeds) return fail(CSSM_EINVAL_ARG, "null argument (desc, theta0, off, t, y, seeds)");
  if (n_iters && (!ll || !theta || !accepted || !last_state)) return fail(CSSM_EINVAL_ARG, "null output");
  if (off[0] != 0) return fail(CSSM_EINVAL_ARG, "off[0] must be 0");
  HostModel probe;
  int rc = cssm_build_model(&probe, desc, false);
  if (rc) return rc;
  if (probe.obs_kind == CSSM_OBS_LGCP)
    return fail(CSSM_EINVAL_DESC, "the fleet does not serve the LGCP observation model (sub-stepped events); " FLEET_PMMH_SERVED);
  size_t flat = 0;
  rc = cssm_desc_flatten(desc, nullptr, 0, &flat);
  if (rc) return rc;
  if (flat != n_theta) return fail(CSSM_EINVAL_ARG, "theta0 has %zu entries per chain, the descriptor flattens to %zu", n_theta, flat);
  if (!f) return fail(CSSM_EINVAL_ARG, "null fleet");
  const uint32_t S = f->S;
  const int d = f->d;
  for (uint32_t k = 0; k < S; ++k) {
    if (off[k + 1] < off[k]) return fail(CSSM_EINVAL_ARG, "off must be non-decreasing (off[%u] = %llu > off[%u] = %llu)", k, (unsigned long long)off[k],
                                         k + 1, (unsigned long long)off[k + 1]);
    if (off[k + 1] == off[k]) return fail(CSSM_EINVAL_ARG, "chain %u has an empty slice of the data (the reference's minBy throws on an empty Vector)", k);
  }
  {   // the structure must be the fleet's: said here, once, not per series of the first iteration
    HostModel same = f->base;
    rc = cssm_build_model(&same, desc, true);
    if (rc) { const std::string keep = cssm_last_error(); return fail(rc, "desc is not of the fleet's model structure (%s); " FLEET_PMMH_SERVED, keep.c_str()); }
  }
  std::vector<cssm_pmmh_chain*> chains(S, nullptr);
  std::vector<const cssm_model_desc*> descs(S);
  std::vector<uint64_t> keys(S);
  std::vector<double> pll(S), last((size_t)S * d);
  std::vector<int> rcs(S);
  for (uint32_t k = 0; k < S && !rc; ++k) rc = cssm_pmmh_chain_create(desc, theta0 + (size_t)k * n_theta, n_theta, delta, seeds[k], d, &chains[k]);
  double split[6] = {0, 0, 0, 0, 0, 0};
  using clk = std::chrono::steady_clock;
  auto ms_since = [](clk::time_point a) { return std::chrono::duration<double, std::milli>(clk::now() - a).count(); };
  for (size_t it = 0; it < n_iters && !rc; ++it) {
    const auto ta = clk::now();
    for (uint32_t k = 0; k < S; ++k) descs[k] = cssm_pmmh_chain_propose(chains[k], it, &keys[k]);
    rc = cssm_fleet_set_params(f, descs.data());
    if (rc) break;
    rc = cssm_fleet_reseed(f, keys.data());
    if (rc) break;
    split[0] += ms_since(ta);
    rc = cssm_fleet_filter(f, off, t, y, has_obs, pll.data(), nullptr, nullptr, nullptr, last.data(), rcs.data());
    if (rc) break;
    split[1] += f->ms_build; split[2] += f->ms_upload; split[3] += f->ms_kernel;
    const auto tc = clk::now();
    for (uint32_t k = 0; k < S; ++k) {
      if (rcs[k] == CSSM_ENONFINITE) pll[k] = -cssm_inf();                    // a proposal the filter cannot weigh is rejected
      else if (rcs[k]) { rc = fail(rcs[k], "chain %u: the fleet's filter returned status %d", k, rcs[k]); break; }
      const size_t o = (size_t)k * n_iters + it;
      cssm_pmmh_chain_decide(chains[k], it, pll[k], last.data() + (size_t)k * d, &ll[o], theta + o * n_theta, &accepted[o], last_state + o * (size_t)d);
    }
    split[4] += ms_since(tc);
    split[5] += 1.0;
  }
  for (cssm_pmmh_chain* c : chains) if (c) cssm_pmmh_chain_destroy(c);
  for (int q = 0; q < 6; ++q) f->pm_split[q] = split[q];
  return rc;
}

extern "C" int cssm_fleet_pmmh_last_split(cssm_fleet* f, double* ms6) {
  if (!f || !ms6) return fail(CSSM_EINVAL_ARG, "null argument");
  for (int q = 0; q < 6; ++q) ms6[q] = f->pm_split[q];
  return CSSM_OK;
}

extern "C" int cssm_fleet_init(cssm_fleet* f, const double* t0) {
  if (!f || !t0) return fail(CSSM_EINVAL_ARG, "null argument");
  HIP_TRY(hipSetDevice(f->device));
  int rc = fleet_ensure(f, 0);
  if (rc) return rc;
  const uint32_t S = f->S;
  unsigned long long* h_off = reinterpret_cast<unsigned long long*>(f->h_stage);
  uint32_t* h_ctl = reinterpret_cast<uint32_t*>(f->h_stage + ((size_t)S + 1u) * 8u);
  for (uint32_t k = 0; k <= S; ++k) h_off[k] = 0;
  for (uint32_t k = 0; k < S; ++k) h_ctl[k] = CSSM_FLEET_CTL_INIT;
  rc = fleet_launch(f, 0, nullptr, nullptr);
  if (rc) return rc;
  for (uint32_t k = 0; k < S; ++k) { f->live[k] = 1; f->t[k] = t0[k]; f->step[k] = 0u; }
  return CSSM_OK;
}

// stepFilter of the active series; iv (cssm_fleet_step_intervals): the same launch also writes getIntervals of every cloud it moved
static int fleet_step_all(cssm_fleet* f, const uint8_t* active, const double* t, const double* y, const uint8_t* has_obs,
                          double* ll_out, int32_t* ess_out, int* rc_out, FleetIv* iv, const FleetIvOut* ivo, FleetFc* fc = nullptr,
                          const FleetFcOut* fco = nullptr, int* fc_rc_out = nullptr) {
  const uint32_t S = f->S;
  bool any_live = false;
  for (uint32_t k = 0; k < S; ++k) any_live = any_live || f->live[k];
  if (!any_live) return fail(CSSM_ESTATE, "no series of the fleet is initialised (cssm_fleet_init / cssm_fleet_ll_filter first)");
  HIP_TRY(hipSetDevice(f->device));
  int rc = fleet_ensure(f, S, false, iv != nullptr, fc != nullptr);
  if (rc) return rc;
  unsigned long long* h_off = reinterpret_cast<unsigned long long*>(f->h_stage);
  uint32_t* h_ctl = reinterpret_cast<uint32_t*>(f->h_stage + ((size_t)S + 1u) * 8u);
  unsigned char* h_recs = f->h_stage + fleet_stage_head(f);
  const size_t RB = CSSM_FLEET_REC_BYTES(f->d);
  size_t R = 0;
  for (uint32_t k = 0; k < S; ++k) {
    h_off[k] = R; h_ctl[k] = 0u;
    if ((!active || active[k]) && f->live[k]) ++R;
  }
  h_off[S] = R;
  fleet_parallel(S, R, [&](size_t lo, size_t hi) {
    for (size_t k = lo; k < hi; ++k)
      if (h_off[k + 1] > h_off[k])
        fleet_pack_rec(f->models[k], f->t[k], t[k], y[k], has_obs ? (int)has_obs[k] : 1, f->step[k], h_recs + (size_t)h_off[k] * RB);
  });
  FleetFcStage fs{nullptr, nullptr, nullptr, nullptr};
  if (fc) {   // the forecast of every active series' record: cssm_fleet_forecast's own refusals of a time, the key, the datum as given
    fs = fleet_fc_stage(f, R);
    fc->step = true; fc->rows = S;
    fc->fc_rc.assign(S, CSSM_OK);
    if (R & 1u) fs.flags[R] = 0u;
    for (uint32_t k = 0; k < S; ++k) {
      const bool runs = h_off[k + 1] > h_off[k];
      fleet_fc_series(f, k, runs, fc, &fs.op[k]);
      if (!runs) continue;
      const size_t r = (size_t)h_off[k];
      const bool on = fc->fc_rc[k] == CSSM_OK && std::isfinite(t[k]) && t[k] >= f->t[k];
      fs.flags[r] = on ? (CSSM_FLEET_FC_ON | ((has_obs ? has_obs[k] : 1) ? CSSM_FLEET_FC_HAS : 0u)) : 0u;
      fs.keys[r] = fc->keys ? fc->keys[k] : cssm_pf_run_key(f->models[k].seed, (1ull << 63) | (uint64_t)f->step[k]);
      fs.y[r] = y[k];
    }
  }
  if (iv) {   // (no launch of a step draws a cloud: the f coefficients of a t0 are not read)
    iv->step = true; iv->rows = S;
    memset(h_recs + R * RB, 0, (size_t)S * f->d * 8u);
  }
  rc = fleet_launch(f, R, nullptr, nullptr, false, nullptr, nullptr, iv, fc);
  if (rc) return rc;
  for (uint32_t k = 0; k < S; ++k) {
    if (fc_rc_out) fc_rc_out[k] = fc->fc_rc[k];
    if (active && !active[k]) { rc_out[k] = CSSM_OK; continue; }            // untouched
    if (!f->live[k]) { rc_out[k] = CSSM_ESTATE; continue; }                 // no cloud: never initialised, or failed since
    const FleetSeries& s = f->h_ser[k];
    if (s.err) { rc_out[k] = CSSM_ENONFINITE; f->live[k] = 0; continue; }
    rc_out[k] = CSSM_OK; f->t[k] = t[k]; f->step[k] += 1u;
    if (ll_out) ll_out[k] = s.ll;
    if (ess_out) ess_out[k] = s.ess;
    if (iv)
      fleet_iv_row(f, k, iv->out.data() + (size_t)k * (f->d + 1) * 3u,
                   reinterpret_cast<const double*>(h_recs + (size_t)h_off[k] * RB + sizeof(FleetRecHead)) + 4 * f->d, *ivo, k);
    if (fc) fleet_fc_row(f, *fc, k, (fs.flags[(size_t)h_off[k]] & CSSM_FLEET_FC_ON) != 0u, *fco, k);
  }
  if (fc && !fc->scale_msg.empty()) (void)fail(CSSM_EINVAL_ARG, "%s", fc->scale_msg.c_str());   // (the call succeeds)
  return CSSM_OK;
}

extern "C" int cssm_fleet_step(cssm_fleet* f, const uint8_t* active, const double* t, const double* y, const uint8_t* has_obs,
                               double* ll_out, int32_t* ess_out, int* rc_out) {
  if (!f || !t || !y || !rc_out) return fail(CSSM_EINVAL_ARG, "null argument");
  return fleet_step_all(f, active, t, y, has_obs, ll_out, ess_out, rc_out, nullptr, nullptr);
}

// filterStream + getIntervals (examples/Filtering.scala:24-31, one observation per sensor per call): cssm_fleet_step, and the summaries of
// every cloud it moved from the same launch.  The entries of a series that is inactive, has no cloud or fails are not written.
extern "C" int cssm_fleet_step_intervals(cssm_fleet* f, const uint8_t* active, const double* t, const double* y, const uint8_t* has_obs, double interval,
                                         double* ll_out, int32_t* ess_out, double* state_mean, double* state_lower, double* state_upper,
                                         double* eta_of_mean, double* eta_lower, double* eta_upper, int* rc_out) {
  if (!t || !y || !rc_out) return fail(CSSM_EINVAL_ARG, "null argument");
  if (!(interval > 0.0 && interval <= 1.0)) return fail(CSSM_EINVAL_ARG, "interval must be in (0, 1]");
  if (!f) return fail(CSSM_EINVAL_ARG, "null fleet");
  FleetIv iv;
  iv.interval = interval;
  const FleetIvOut o{state_mean, state_lower, state_upper, eta_of_mean, eta_lower, eta_upper};
  return fleet_step_all(f, active, t, y, has_obs, ll_out, ess_out, rc_out, &iv, &o);
}

// getMeanForecast over a filterStream, one observation per sensor per call: cssm_fleet_step -- the same arguments, bits and statuses -- and
// before the record is stepped cssm_fleet_forecast of its time, from the same launch.  The entries of a series that is inactive, has no
// cloud or fails are not written.
extern "C" int cssm_fleet_step_forecast(cssm_fleet* f, const uint8_t* active, const double* t, const double* y, const uint8_t* has_obs,
                                        const uint64_t* keys, double interval, double* ll_out, int32_t* ess_out, double* state_mean,
                                        double* state_lower, double* state_upper, double* eta_mean, double* eta_lower, double* eta_upper,
                                        double* obs_mean, double* obs_lower, double* obs_upper, int32_t* obs_below, int32_t* obs_equal,
                                        int* rc_out, int* fc_rc_out) {
  if (!t || !y || !rc_out || !fc_rc_out) return fail(CSSM_EINVAL_ARG, "null argument (t, y, rc_out, fc_rc_out)");
  if (!(interval > 0.0 && interval <= 1.0)) return fail(CSSM_EINVAL_ARG, "interval must be in (0, 1]");
  if (!f) return fail(CSSM_EINVAL_ARG, "null fleet");
  FleetFc fc;
  fc.interval = interval; fc.keys = keys;
  const FleetFcOut o{state_mean, state_lower, state_upper, eta_mean, eta_lower, eta_upper, obs_mean, obs_lower, obs_upper, obs_below, obs_equal};
  return fleet_step_all(f, active, t, y, has_obs, ll_out, ess_out, rc_out, nullptr, nullptr, &fc, &o, fc_rc_out);
}

extern "C" int cssm_fleet_summary(cssm_fleet* f, double interval, double* state_mean, double* state_lower, double* state_upper,
                                  double* eta_of_mean, double* eta_lower, double* eta_upper) {
  if (!f) return fail(CSSM_EINVAL_ARG, "null fleet");
  if (!(interval > 0.0 && interval <= 1.0)) return fail(CSSM_EINVAL_ARG, "interval must be in (0, 1]");
  HIP_TRY(hipSetDevice(f->device));
  const uint32_t S = f->S, n = f->n;
  const int d = f->d, rows = d + 1;
  // layout of d_sm (doubles): [S][d] f coefficients | [S][rows][3] results | [S] buffer numbers (u32, two per double)
  const size_t n_fco = (size_t)S * d, n_out = (size_t)S * rows * 3, n_cur = ((size_t)S + 1) / 2, need = n_fco + n_out + n_cur;
  if (need > f->sm_cap) {
    if (f->d_sm) (void)hipFree(f->d_sm);
    f->d_sm = nullptr; f->sm_cap = 0;
    if (hipMalloc(&f->d_sm, need * 8) != hipSuccess) return fail(CSSM_ENOMEM, "fleet summary buffers");
    f->sm_cap = need;
  }
  std::vector<double> hbuf(need, 0.0);
  uint32_t* hcur = reinterpret_cast<uint32_t*>(hbuf.data() + n_fco + n_out);
  fleet_parallel(S, (size_t)S * 4, [&](size_t lo, size_t hi) {
    for (size_t k = lo; k < hi; ++k) {
      StepRec r;
      cssm_build_rec(&f->models[k], f->t[k], f->t[k], 0.0, 0, f->step[k], &r);   // F(t) of the series' own time
      for (int c = 0; c < d; ++c) hbuf[k * d + c] = r.fco[c];
      hcur[k] = f->live[k] ? (f->step[k] & 1u) : 0xffffffffu;
    }
  });
  SelState rs, re;   // the ranks of a state row and of the eta row, as cssm_pf_summary takes them
  sel_ranks(rs, n, interval, true);
  sel_ranks(re, n, interval, false);
  uint32_t np2 = 2u;
  while (np2 < n) np2 <<= 1;
  double* d_fco = f->d_sm; double* d_out = f->d_sm + n_fco;
  const uint32_t* d_cur = reinterpret_cast<const uint32_t*>(f->d_sm + n_fco + n_out);
  HIP_TRY(hipEventRecord(f->ev[2], f->stream));
  HIP_TRY(hipMemcpyAsync(f->d_sm, hbuf.data(), need * 8, hipMemcpyHostToDevice, f->stream));
  DISPATCH_D(d, hipLaunchKernelGGL(k_fleet_summary<D>, dim3(S, rows), dim3(CSSM_BLOCK), (size_t)np2 * 8u, f->stream, f->state, f->anc, d_cur, d_fco, n, np2,
                                   f->base.mk, (uint32_t)rs.rank[0], (uint32_t)rs.rank[1], (uint32_t)re.rank[0], (uint32_t)re.rank[1], d_out));
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(hbuf.data() + n_fco, d_out, n_out * 8, hipMemcpyDeviceToHost, f->stream));
  HIP_TRY(hipEventRecord(f->ev[3], f->stream));
  HIP_TRY(hipStreamSynchronize(f->stream));
  if (hipEventElapsedTime(&f->ms_summary, f->ev[2], f->ev[3]) != hipSuccess) f->ms_summary = -1.f;
  const double* ho = hbuf.data() + n_fco;
  for (uint32_t k = 0; k < S; ++k) {
    double mean[CSSM_MAX_DIM];
    for (int c = 0; c < d; ++c) {
      const double* o = ho + ((size_t)k * rows + c) * 3;
      mean[c] = o[0];
      if (state_mean) state_mean[(size_t)k * d + c] = o[0];
      if (state_lower) state_lower[(size_t)k * d + c] = o[1];
      if (state_upper) state_upper[(size_t)k * d + c] = o[2];
    }
    const double* oe = ho + ((size_t)k * rows + d) * 3;
    if (eta_lower) eta_lower[k] = oe[1];
    if (eta_upper) eta_upper[k] = oe[2];
    if (eta_of_mean) eta_of_mean[k] = f->live[k] ? cssm_eta_of_mean(f->models[k], hbuf.data() + (size_t)k * d, mean) : cssm_nan();   // :420
  }
  return CSSM_OK;
}

// SimulateData.forecast + summariseForecast (model/Data.scala:196-231) of every series from its current cloud: one upload (offsets,
// keys, observation parameters, buffer numbers, records), one launch whose blocks are the series (k_fleet_forecast), one read-back.
// A call that returns samples runs the fleet in chunks of series whose samples fit fc_samp_max -- never chunks of horizons: a series
// is one block's work.  What a series' own arguments spoil is the series' own: its status, NaN in its outputs, no block for it.
// the grow-only buffers of both forecasts: `need` bytes of d_fc and of its pinned mirror, 16 N bytes of eta / obs staging per series
static int fleet_fc_ensure(cssm_fleet* f, size_t need) {
  if (need > f->h_fc_cap) {
    if (f->h_fc) (void)hipHostFree(f->h_fc);
    f->h_fc = nullptr; f->h_fc_cap = 0;
    if (hipHostMalloc((void**)&f->h_fc, need + need / 4, hipHostMallocDefault) != hipSuccess) return fail(CSSM_ENOMEM, "fleet forecast: %zu bytes of pinned staging", need);
    f->h_fc_cap = need + need / 4;
  }
  if (need > f->fc_cap) {
    if (f->d_fc) (void)hipFree(f->d_fc);
    f->d_fc = nullptr; f->fc_cap = 0;
    if (hipMalloc(&f->d_fc, need + need / 4) != hipSuccess) return fail(CSSM_ENOMEM, "fleet forecast: %zu bytes of records and results", need);
    f->fc_cap = need + need / 4;
  }
  if (!f->d_fc_stage && hipMalloc(&f->d_fc_stage, (size_t)f->S * 2u * f->n * 8u) != hipSuccess) {
    f->d_fc_stage = nullptr;
    return fail(CSSM_ENOMEM, "fleet forecast: 16 N bytes of staging per series");
  }
  return CSSM_OK;
}

// chunks of series [cut[c], cut[c + 1]): all of them, or (samples) as many as fit the cap -- one series at least; the device buffer
// of one chunk's samples
static int fleet_fc_cuts(cssm_fleet* f, const uint64_t* off, bool samples, std::vector<uint32_t>& cut) {
  const uint32_t S = f->S;
  const size_t samp_row = (size_t)(f->d + 3) * f->n * 8u;
  cut.assign(1, 0u);
  if (!samples) { cut.push_back(S); return CSSM_OK; }
  const size_t cap_rows = std::max<size_t>(1, f->fc_samp_max / samp_row);
  size_t most = 0;
  for (uint32_t k = 0; k < S; ++k)
    if ((size_t)(off[k + 1] - off[cut.back()]) > cap_rows && k > cut.back()) cut.push_back(k);
  cut.push_back(S);
  for (size_t c = 0; c + 1 < cut.size(); ++c) most = std::max<size_t>(most, (size_t)(off[cut[c + 1]] - off[cut[c]]));
  if (most * samp_row > f->fc_samp_cap) {
    if (f->d_fc_samp) (void)hipFree(f->d_fc_samp);
    f->d_fc_samp = nullptr; f->fc_samp_cap = 0;
    if (hipMalloc(&f->d_fc_samp, most * samp_row) != hipSuccess) return fail(CSSM_ENOMEM, "fleet forecast: %zu bytes of samples", most * samp_row);
    f->fc_samp_cap = most * samp_row;
  }
  return CSSM_OK;
}

// what every launch of either forecast kernel shares: sizes, ranks, the way to a row's order statistics, the fleet's buffers
static void fleet_fc_args(const cssm_fleet* f, double interval, FleetFcLaunch& l) {
  const uint32_t n = f->n;
  SelState rs, re;
  sel_ranks(rs, n, interval, true);
  sel_ranks(re, n, interval, false);
  l.args.n = n; l.args.np2 = 2u;
  while (l.args.np2 < n) l.args.np2 <<= 1;
  l.args.select = f->fc_select ? (uint32_t)(f->fc_select == 2) : (uint32_t)(n >= CSSM_FLEET_SELECT_MIN_N);
  l.args.state = f->state; l.args.anc = f->anc;
  l.args.stage = f->d_fc_stage;
  l.args.logtab = f->logtab; l.args.mk = f->base.mk;
  l.args.lo_state = (uint32_t)rs.rank[0]; l.args.hi_state = (uint32_t)rs.rank[1];
  l.args.lo_eta = (uint32_t)re.rank[0]; l.args.hi_eta = (uint32_t)re.rank[1];
  l.d = f->d; l.threads = f->threads; l.stream = f->stream;
}

// the results [R][d + 2][3] into the caller's arrays; a series whose status is not zero reads NaN
static void fleet_fc_scatter(const cssm_fleet* f, const uint64_t* off, const double* h_out, const int* rc_out, double* state_mean, double* state_lower,
                             double* state_upper, double* eta_mean, double* eta_lower, double* eta_upper, double* obs_mean, double* obs_lower,
                             double* obs_upper, double* samples) {
  const uint32_t n = f->n;
  const int d = f->d, rows = d + 2;
  for (uint32_t k = 0; k < f->S; ++k) {
    const bool ok = rc_out[k] == CSSM_OK;
    for (size_t r = (size_t)off[k]; r < (size_t)off[k + 1]; ++r) {
      const double* o = h_out + r * (size_t)rows * 3u;
      auto at = [&](int row, int q) { return ok ? o[3 * row + q] : cssm_nan(); };
      for (int c = 0; c < d; ++c) {
        if (state_mean) state_mean[r * d + c] = at(c, 0);
        if (state_lower) state_lower[r * d + c] = at(c, 1);
        if (state_upper) state_upper[r * d + c] = at(c, 2);
      }
      if (eta_mean) eta_mean[r] = at(d, 0);
      if (eta_lower) eta_lower[r] = at(d, 1);
      if (eta_upper) eta_upper[r] = at(d, 2);
      if (obs_mean) obs_mean[r] = at(d + 1, 0);
      if (obs_lower) obs_lower[r] = at(d + 1, 1);
      if (obs_upper) obs_upper[r] = at(d + 1, 2);
      if (samples && !ok) std::fill(samples + r * (size_t)(d + 3) * n, samples + (r + 1) * (size_t)(d + 3) * n, cssm_nan());
    }
  }
}

// upload `up` bytes of the staged call, run it in the chunks of series `cut` (launch(l) starts one chunk's kernel), bring the samples of
// every chunk and the bytes [back, back + back_bytes) of d_fc home; the device time lands in ms_forecast
template <class Launch>
static int fleet_fc_run(cssm_fleet* f, const uint64_t* off, const std::vector<uint32_t>& cut, FleetFcLaunch& l, size_t up, size_t back, size_t back_bytes,
                        double* samples, const char* kernel, Launch&& launch) {
  const size_t samp_row = (size_t)(f->d + 3) * f->n * 8u;
  HIP_TRY(hipEventRecord(f->ev[4], f->stream));
  HIP_TRY(hipMemcpyAsync(f->d_fc, f->h_fc, up, hipMemcpyHostToDevice, f->stream));
  for (size_t c = 0; c + 1 < cut.size(); ++c) {
    const size_t ra = (size_t)off[cut[c]], rb = (size_t)off[cut[c + 1]];
    if (rb == ra) continue;
    l.args.k0 = cut[c]; l.n_series = cut[c + 1] - cut[c];
    l.args.samples = samples ? f->d_fc_samp : nullptr; l.args.samp_r0 = ra;
    const int hrc = launch(l);
    if (hrc) return fail(CSSM_EHIP, "%s: %s", kernel, hipGetErrorString((hipError_t)hrc));
    if (samples) HIP_TRY(hipMemcpyAsync(samples + ra * (size_t)(f->d + 3) * f->n, f->d_fc_samp, (rb - ra) * samp_row, hipMemcpyDeviceToHost, f->stream));
    if (samples && c + 2 < cut.size()) HIP_TRY(hipStreamSynchronize(f->stream));   // (the next chunk writes the same buffer)
  }
  HIP_TRY(hipMemcpyAsync(f->h_fc + back, f->d_fc + back, back_bytes, hipMemcpyDeviceToHost, f->stream));
  HIP_TRY(hipEventRecord(f->ev[5], f->stream));
  HIP_TRY(hipStreamSynchronize(f->stream));
  if (hipEventElapsedTime(&f->ms_forecast, f->ev[4], f->ev[5]) != hipSuccess) f->ms_forecast = -1.f;
  return CSSM_OK;
}

extern "C" int cssm_fleet_forecast(cssm_fleet* f, const uint64_t* off, const double* t, const uint64_t* keys, double interval,
                                   double* state_mean, double* state_lower, double* state_upper, double* eta_mean, double* eta_lower,
                                   double* eta_upper, double* obs_mean, double* obs_lower, double* obs_upper, double* samples, int* rc_out) {
  if (!f || !off || !t || !keys || !rc_out) return fail(CSSM_EINVAL_ARG, "null argument");
  const uint32_t S = f->S;
  if (off[0] != 0) return fail(CSSM_EINVAL_ARG, "off[0] must be 0");
  for (uint32_t k = 0; k < S; ++k)
    if (off[k + 1] < off[k]) return fail(CSSM_EINVAL_ARG, "off must be non-decreasing (off[%u] = %llu > off[%u] = %llu)", k, (unsigned long long)off[k],
                                         k + 1, (unsigned long long)off[k + 1]);
  if (!(interval > 0.0 && interval <= 1.0)) return fail(CSSM_EINVAL_ARG, "interval must be in (0, 1]");
  const size_t R = (size_t)off[S];
  for (uint32_t k = 0; k < S; ++k)
    if (off[k + 1] - off[k] > 0xffffffffull) return fail(CSSM_EINVAL_ARG, "series %u: too many horizons", k);
  if (R == 0) { for (uint32_t k = 0; k < S; ++k) rc_out[k] = CSSM_OK; return CSSM_OK; }
  bool any_live = false;
  for (uint32_t k = 0; k < S; ++k) any_live = any_live || f->live[k];
  if (!any_live) return fail(CSSM_ESTATE, "no series of the fleet is initialised (cssm_fleet_init / cssm_fleet_ll_filter first)");
  HIP_TRY(hipSetDevice(f->device));
  const int d = f->d, rows = d + 2;
  const size_t RB = CSSM_FLEET_REC_BYTES(d);
  const size_t o_keys = ((size_t)S + 1u) * 8u, o_op = o_keys + (size_t)S * 8u, o_cur = o_op + (size_t)S * sizeof(cssm_obs_params);
  const size_t o_rec = o_cur + (((size_t)S * 4u + 7u) & ~(size_t)7u), o_out = o_rec + R * RB, n_out = R * (size_t)rows * 3u;
  const size_t need = o_out + n_out * 8u;
  {
    const int erc = fleet_fc_ensure(f, need);
    if (erc) return erc;
  }
  unsigned long long* h_off = reinterpret_cast<unsigned long long*>(f->h_fc);
  unsigned long long* h_keys = reinterpret_cast<unsigned long long*>(f->h_fc + o_keys);
  cssm_obs_params* h_op = reinterpret_cast<cssm_obs_params*>(f->h_fc + o_op);
  uint32_t* h_cur = reinterpret_cast<uint32_t*>(f->h_fc + o_cur);
  unsigned char* h_recs = f->h_fc + o_rec;
  const double* h_out = reinterpret_cast<const double*>(f->h_fc + o_out);
  // the series' own statuses: no cloud, a model without the scale its observation needs, times that are not a forecast's
  std::string scale_msg;
  size_t n_run = 0;
  for (uint32_t k = 0; k <= S; ++k) h_off[k] = off[k];
  for (uint32_t k = 0; k < S; ++k) {
    const size_t a = (size_t)off[k], b = (size_t)off[k + 1];
    h_keys[k] = keys[k]; h_cur[k] = 0xffffffffu; rc_out[k] = CSSM_OK;
    memset(&h_op[k], 0, sizeof(cssm_obs_params));
    if (b == a) continue;
    if (!f->live[k]) { rc_out[k] = CSSM_ESTATE; continue; }
    if (cssm_obs_params_or_fail(f->base.obs_kind, f->obs_has_scale[k], f->obs_scale[k], f->base.obs_df, &h_op[k])) {
      if (scale_msg.empty()) scale_msg = "series " + std::to_string(k) + ": " + cssm_last_error();
      rc_out[k] = CSSM_EINVAL_ARG;
      continue;
    }
    double prev = f->t[k];
    for (size_t s = a; s < b; ++s) {
      if (!std::isfinite(t[s]) || !(t[s] >= prev)) { rc_out[k] = CSSM_EINVAL_ARG; break; }
      prev = t[s];
    }
    if (rc_out[k]) continue;
    h_cur[k] = f->step[k] & 1u;
    n_run += b - a;
  }
  fleet_parallel(S, n_run, [&](size_t lo, size_t hi) {
    for (size_t k = lo; k < hi; ++k) {
      if (h_cur[k] > 1u) continue;
      double tp = f->t[k];
      for (size_t s = (size_t)off[k]; s < (size_t)off[k + 1]; ++s) {
        fleet_pack_rec(f->models[k], tp, t[s], 0.0, 0, (uint32_t)(s - (size_t)off[k]), h_recs + s * RB);
        tp = t[s];
      }
    }
  });
  if (n_run) {
    std::vector<uint32_t> cut;
    int rc = fleet_fc_cuts(f, off, samples != nullptr, cut);
    if (rc) return rc;
    FleetFcLaunch l;
    fleet_fc_args(f, interval, l);
    l.args.off = reinterpret_cast<const unsigned long long*>(f->d_fc);
    l.args.keys = reinterpret_cast<const unsigned long long*>(f->d_fc + o_keys);
    l.args.op = reinterpret_cast<const cssm_obs_params*>(f->d_fc + o_op);
    l.args.cur = reinterpret_cast<const uint32_t*>(f->d_fc + o_cur);
    l.args.recs = f->d_fc + o_rec;
    l.args.out = reinterpret_cast<double*>(f->d_fc + o_out);
    rc = fleet_fc_run(f, off, cut, l, o_out, o_out, n_out * 8u, samples, "k_fleet_forecast", [](const FleetFcLaunch& q) { return cssm_fleet_forecast_launch(q); });
    if (rc) return rc;
  }
  fleet_fc_scatter(f, off, h_out, rc_out, state_mean, state_lower, state_upper, eta_mean, eta_lower, eta_upper, obs_mean, obs_lower, obs_upper, samples);
  if (!scale_msg.empty()) (void)fail(CSSM_EINVAL_ARG, "%s", scale_msg.c_str());   // (the call succeeds; the message names the first such series)
  return CSSM_OK;
}

// SimulateData.forecast(unparamModel, t, n)(posterior) + summariseForecast of every series under its OWN joint posterior sample
// (cssm_pf_forecast_posterior per series): the rows of every series validated and constraint-transformed by cssm_posterior_rows on a
// few host threads, then one upload (offsets, keys, buffer numbers, records, states, rows, the caller's picks), one launch per chunk
// of series (k_fleet_forecast_post), one read-back (the picks, the results).  The fleet lends its device, stream, contract table, N,
// structure and scratch -- the state buffer of a series that does not hold its cloud among it; nothing it keeps per series changes.
extern "C" int cssm_fleet_forecast_posterior(cssm_fleet* f, const cssm_model_desc* desc, const uint64_t* moff, const double* theta, size_t n_theta,
                                             const double* x, const double* t0, const uint64_t* off, const double* t, const uint32_t* pick,
                                             const uint64_t* keys, double interval, double* state_mean, double* state_lower, double* state_upper,
                                             double* eta_mean, double* eta_lower, double* eta_upper, double* obs_mean, double* obs_lower,
                                             double* obs_upper, double* samples, uint32_t* pick_out, int* rc_out) {
  if (!f || !desc || !moff || !theta || !x || !t0 || !off || !t || !keys || !rc_out) return fail(CSSM_EINVAL_ARG, "null argument");
  const uint32_t S = f->S, n = f->n;
  if (moff[0] != 0) return fail(CSSM_EINVAL_ARG, "moff[0] must be 0");
  if (off[0] != 0) return fail(CSSM_EINVAL_ARG, "off[0] must be 0");
  for (uint32_t k = 0; k < S; ++k) {
    if (moff[k + 1] < moff[k]) return fail(CSSM_EINVAL_ARG, "moff must be non-decreasing (moff[%u] = %llu > moff[%u] = %llu)", k,
                                           (unsigned long long)moff[k], k + 1, (unsigned long long)moff[k + 1]);
    if (off[k + 1] < off[k]) return fail(CSSM_EINVAL_ARG, "off must be non-decreasing (off[%u] = %llu > off[%u] = %llu)", k, (unsigned long long)off[k],
                                         k + 1, (unsigned long long)off[k + 1]);
  }
  if (!(interval > 0.0 && interval <= 1.0)) return fail(CSSM_EINVAL_ARG, "interval must be in (0, 1]");
  if (!desc->leaves || desc->n_leaves < 1) return fail(CSSM_EINVAL_DESC, "null model descriptor");
  {   // the structure (an LGCP descriptor is never a fleet's) and the length of a row: no rows looked at
    const int rc = cssm_posterior_rows_into(&f->base, desc, theta, n_theta, 0, nullptr);
    if (rc) return rc;
  }
  const size_t R = (size_t)off[S], Mtot = (size_t)moff[S];
  const int d = f->d, rows = d + 2;
  const size_t RS = 3 * (size_t)d + 1, RB = CSSM_FLEET_REC_BYTES(d);
  HIP_TRY(hipSetDevice(f->device));
  // layout: [off | keys | moff | buffer numbers | records | x | rows | picks | results]; the caller's picks are uploaded, the drawn
  // ones only read back
  const size_t o_keys = ((size_t)S + 1u) * 8u, o_moff = o_keys + (size_t)S * 8u, o_cur = o_moff + ((size_t)S + 1u) * 8u;
  const size_t o_rec = o_cur + (((size_t)S * 4u + 7u) & ~(size_t)7u), o_x = o_rec + R * RB, o_rows = o_x + Mtot * (size_t)d * 8u;
  const size_t o_pick = o_rows + Mtot * RS * 8u, o_out = o_pick + (((size_t)S * n * 4u + 7u) & ~(size_t)7u), n_out = R * (size_t)rows * 3u;
  const size_t need = o_out + n_out * 8u;
  int rc = fleet_fc_ensure(f, need);
  if (rc) return rc;
  unsigned long long* h_off = reinterpret_cast<unsigned long long*>(f->h_fc);
  unsigned long long* h_keys = reinterpret_cast<unsigned long long*>(f->h_fc + o_keys);
  unsigned long long* h_moff = reinterpret_cast<unsigned long long*>(f->h_fc + o_moff);
  uint32_t* h_cur = reinterpret_cast<uint32_t*>(f->h_fc + o_cur);
  unsigned char* h_recs = f->h_fc + o_rec;
  double* h_x = reinterpret_cast<double*>(f->h_fc + o_x);                  // (a series' states are copied here once they are known finite)
  double* h_rows = reinterpret_cast<double*>(f->h_fc + o_rows);
  uint32_t* h_pick = reinterpret_cast<uint32_t*>(f->h_fc + o_pick);
  const double* h_out = reinterpret_cast<const double*>(f->h_fc + o_out);
  for (uint32_t k = 0; k <= S; ++k) { h_off[k] = off[k]; h_moff[k] = moff[k]; }
  if (pick) memcpy(h_pick, pick, (size_t)S * n * 4u);
  // the series' own statuses (what cssm_pf_forecast_posterior refuses, in its order); the message of each as its thread left it
  cssm_obs_params op;
  std::string scale_msg;
  const bool no_scale = cssm_obs_params_or_fail(f->base.obs_kind, desc->leaves[0].has_scale, desc->leaves[0].scale, f->base.obs_df, &op) != 0;
  if (no_scale) scale_msg = cssm_last_error();
  std::vector<std::string> msg(S);
  fleet_parallel(S, Mtot + R, [&](size_t lo, size_t hi) {
    for (size_t k = lo; k < hi; ++k) {
      const size_t ha = (size_t)off[k], hb = (size_t)off[k + 1], ma = (size_t)moff[k], M = (size_t)moff[k + 1] - ma;
      h_keys[k] = keys[k]; h_cur[k] = 0xffffffffu; rc_out[k] = CSSM_OK;
      auto refuse = [&](const std::string& why) { rc_out[k] = CSSM_EINVAL_ARG; msg[k] = why; };
      if (M == 0) {
        if (hb > ha) refuse("the posterior sample is empty (M = 0)");
        continue;
      }
      if (M > 0xffffffffull) { refuse("the posterior sample has more than 2^32 - 1 rows"); continue; }
      if (hb - ha > 0xffffffffull) { refuse("too many horizons"); continue; }
      if (!std::isfinite(t0[k])) { refuse("t0 is not finite"); continue; }
      if (no_scale) { refuse(scale_msg); continue; }             // (with or without horizons, as the single handle)
      if (cssm_posterior_rows_into(&f->base, desc, theta + ma * n_theta, n_theta, M, h_rows + ma * RS)) { refuse(cssm_last_error()); continue; }
      const double* xs = x + ma * (size_t)d;
      for (size_t m = 0; m < M && !rc_out[k]; ++m)
        for (int c = 0; c < d; ++c)
          if (!std::isfinite(xs[m * d + c])) { refuse("x row " + std::to_string(m) + ": component " + std::to_string(c) + " is not finite"); break; }
      if (rc_out[k]) continue;
      memcpy(h_x + ma * (size_t)d, xs, M * (size_t)d * 8u);
      if (pick)
        for (uint32_t i = 0; i < n; ++i)
          if (pick[(size_t)k * n + i] >= M) {
            refuse("pick[" + std::to_string(i) + "] = " + std::to_string(pick[(size_t)k * n + i]) + " is not below M = " + std::to_string(M));
            break;
          }
      if (rc_out[k]) continue;
      double prev = t0[k];
      for (size_t s = ha; s < hb; ++s) {
        if (!std::isfinite(t[s])) { refuse("t[" + std::to_string(s - ha) + "] is not finite"); break; }
        if (!(t[s] >= prev)) { refuse(s > ha ? "t must be non-decreasing" : "t[0] is before t0"); break; }
        prev = t[s];
      }
      if (rc_out[k] || hb == ha) continue;
      h_cur[k] = f->live[k] ? (f->step[k] & 1u) : 0u;          // the cloud's buffer is only named to be avoided; without a cloud both are free
      double tp = t0[k];
      for (size_t s = ha; s < hb; ++s) {
        fleet_pack_rec(f->models[k], tp, t[s], 0.0, 0, (uint32_t)(s - ha), h_recs + s * RB);
        tp = t[s];
      }
    }
  });
  size_t n_run = 0;
  for (uint32_t k = 0; k < S; ++k)
    if (h_cur[k] <= 1u) n_run += (size_t)(off[k + 1] - off[k]);
  if (n_run) {
    std::vector<uint32_t> cut;
    rc = fleet_fc_cuts(f, off, samples != nullptr, cut);
    if (rc) return rc;
    FleetFcLaunch l;
    fleet_fc_args(f, interval, l);
    l.args.off = reinterpret_cast<const unsigned long long*>(f->d_fc);
    l.args.keys = reinterpret_cast<const unsigned long long*>(f->d_fc + o_keys);
    l.args.op = nullptr;
    l.args.cur = reinterpret_cast<const uint32_t*>(f->d_fc + o_cur);
    l.args.recs = f->d_fc + o_rec;
    l.args.out = reinterpret_cast<double*>(f->d_fc + o_out);
    FleetFcPost q;
    q.moff = reinterpret_cast<const unsigned long long*>(f->d_fc + o_moff);
    q.x = reinterpret_cast<const double*>(f->d_fc + o_x);
    q.rows = reinterpret_cast<const double*>(f->d_fc + o_rows);
    q.picks = reinterpret_cast<uint32_t*>(f->d_fc + o_pick);
    q.draw = pick ? 0u : 1u;
    q.obs_df = f->base.obs_df;
    const size_t back = pick_out && !pick ? o_pick : o_out;
    rc = fleet_fc_run(f, off, cut, l, pick ? o_out : o_pick, back, need - back, samples, "k_fleet_forecast_post",
                      [&](const FleetFcLaunch& ll) { return cssm_fleet_forecast_post_launch(ll, q); });
    if (rc) return rc;
  }
  fleet_fc_scatter(f, off, h_out, rc_out, state_mean, state_lower, state_upper, eta_mean, eta_lower, eta_upper, obs_mean, obs_lower, obs_upper, samples);
  if (pick_out)   // a series that ran: what its block used; one without horizons: the same picks, formed here; a refused or empty one: zeros
    for (uint32_t k = 0; k < S; ++k) {
      uint32_t* po = pick_out + (size_t)k * n;
      const uint64_t M = moff[k + 1] - moff[k];
      if (rc_out[k] || M == 0) { std::fill(po, po + n, 0u); continue; }
      if (pick) { memcpy(po, pick + (size_t)k * n, (size_t)n * 4u); continue; }
      if (h_cur[k] <= 1u) { memcpy(po, h_pick + (size_t)k * n, (size_t)n * 4u); continue; }
      for (uint32_t i = 0; i < n; ++i) po[i] = cssm_posterior_pick(keys[k], i, M);
    }
  for (uint32_t k = 0; k < S; ++k)   // (the call succeeds; the message names the first refused series)
    if (rc_out[k]) { (void)fail(CSSM_EINVAL_ARG, "series %u: %s", k, msg[k].c_str()); break; }
  return CSSM_OK;
}

// FilterInterpolate (model/ParticleFilter.scala:273-311, examples/Interpolate.scala:31-44) of every series: cssm_pf_interpolate per
// series in TWO launches per chunk of series -- the forward pass keeps every cloud and every weighted record's ancestors of a series
// in a slab of its own (k_fleet_series<D, false, true>), the backward pass composes the surviving lineages and summarises every time
// index (k_fleet_lineage, cssm_fleet_interp.hip).  The fleet lends its device, stream, contract table, N, structure, parameters and
// keys; nothing it keeps per series changes.  Chunks: as many series as fit ip_hist_max bytes of history, one at least -- never a
// part of a series.  Per chunk one upload (offsets, records, the f coefficients of every output row), the two launches, one read-back.
extern "C" int cssm_fleet_interpolate(cssm_fleet* f, const uint64_t* off, const double* t, const double* y, const uint8_t* has_obs, double interval,
                                      int flags, double* ll_out, double* state_mean, double* state_lower, double* state_upper, double* eta_of_mean,
                                      double* eta_lower, double* eta_upper, int* rc_out) {
  if (!off) return fail(CSSM_EINVAL_ARG, "off is null");
  if (!ll_out || !rc_out) return fail(CSSM_EINVAL_ARG, "ll_out / rc_out is null");
  if (off[0] != 0) return fail(CSSM_EINVAL_ARG, "off[0] must be 0");
  if (!t || !y) return fail(CSSM_EINVAL_ARG, "null data");
  if (!(interval > 0.0 && interval <= 1.0)) return fail(CSSM_EINVAL_ARG, "interval must be in (0, 1]");
  if (flags & ~CSSM_INTERP_REFERENCE_PAIRING) return fail(CSSM_EINVAL_ARG, "unknown flag bits 0x%x (CSSM_INTERP_REFERENCE_PAIRING is the only flag)",
                                                          (unsigned)(flags & ~CSSM_INTERP_REFERENCE_PAIRING));
  if (!f) return fail(CSSM_EINVAL_ARG, "null fleet");
  const uint32_t S = f->S, n = f->n;
  const int d = f->d, rows = d + 1;
  for (uint32_t k = 0; k < S; ++k) {
    if (off[k + 1] < off[k]) return fail(CSSM_EINVAL_ARG, "off must be non-decreasing (off[%u] = %llu > off[%u] = %llu)", k, (unsigned long long)off[k],
                                         k + 1, (unsigned long long)off[k + 1]);
    if (off[k + 1] - off[k] > 0xfffffffeull) return fail(CSSM_EINVAL_ARG, "series %u: too many records", k);
  }
  HIP_TRY(hipSetDevice(f->device));
  int rc = fleet_upload_par(f);
  if (rc) return rc;
  // chunks of series [cut[c], cut[c + 1]) whose history fits the cap; the buffers of the largest one
  const size_t RB = CSSM_FLEET_REC_BYTES(d), slice = (size_t)n * (8u * (size_t)d + 4u);
  auto stage_o = [&](uint32_t k0, uint32_t k1, size_t* o) {   // byte offsets of [off | recs | fco | ser | out | end] of a chunk
    const size_t Sc = k1 - k0, Rc = (size_t)(off[k1] - off[k0]), Qc = Rc + Sc;
    o[0] = 0; o[1] = (Sc + 1u) * 8u; o[2] = o[1] + Rc * RB; o[3] = o[2] + Qc * (size_t)d * 8u; o[4] = o[3] + Sc * sizeof(FleetSeries);
    o[5] = o[4] + Qc * (size_t)rows * 24u;
  };
  std::vector<uint32_t> cut(1, 0u);
  size_t held = 0, need = 0, need_hist = 0;
  uint32_t widest = 0;
  for (uint32_t k = 0; k < S; ++k) {
    const size_t b = ((size_t)(off[k + 1] - off[k]) + 1u) * slice;
    if (k > cut.back() && held + b > f->ip_hist_max) { cut.push_back(k); held = 0; }
    held += b;
    if (held > need_hist) { need_hist = held; widest = cut.back(); }
  }
  cut.push_back(S);
  for (size_t c = 0; c + 1 < cut.size(); ++c) {
    size_t o[6];
    stage_o(cut[c], cut[c + 1], o);
    need = std::max(need, o[5]);
  }
  if (need > f->h_ip_cap) {
    if (f->h_ip) (void)hipHostFree(f->h_ip);
    f->h_ip = nullptr; f->h_ip_cap = 0;
    if (hipHostMalloc((void**)&f->h_ip, need + need / 4, hipHostMallocDefault) != hipSuccess) return fail(CSSM_ENOMEM, "fleet interpolation: %zu bytes of pinned staging", need);
    f->h_ip_cap = need + need / 4;
  }
  if (need > f->ip_cap) {
    if (f->d_ip) (void)hipFree(f->d_ip);
    f->d_ip = nullptr; f->ip_cap = 0;
    if (hipMalloc(&f->d_ip, need + need / 4) != hipSuccess) return fail(CSSM_ENOMEM, "fleet interpolation: %zu bytes of records and results", need);
    f->ip_cap = need + need / 4;
  }
  if (need_hist > f->ip_hist_cap) {
    if (f->d_ip_hist) (void)hipFree(f->d_ip_hist);
    f->d_ip_hist = nullptr; f->ip_hist_cap = 0;
    if (hipMalloc(&f->d_ip_hist, need_hist) != hipSuccess) {
      f->d_ip_hist = nullptr;
      if (need_hist > f->ip_hist_max)   // a series longer than the cap runs alone
        return fail(CSSM_ENOMEM, "fleet interpolation: series %u alone needs %zu bytes of lineage history ((T + 1) N (8 d + 4))", widest, need_hist);
      return fail(CSSM_ENOMEM, "fleet interpolation: %zu bytes of lineage history (CSSM_OPT_INTERP_CAP lowers it)", need_hist);
    }
    f->ip_hist_cap = need_hist;
  }
  SelState rs, re;
  sel_ranks(rs, n, interval, true);
  sel_ranks(re, n, interval, false);
  uint32_t np2 = 2u;
  while (np2 < n) np2 <<= 1;
  const bool pairing = (flags & CSSM_INTERP_REFERENCE_PAIRING) != 0;
  double ms[2] = {0.0, 0.0};
  for (size_t c = 0; c + 1 < cut.size(); ++c) {
    const uint32_t k0 = cut[c], k1 = cut[c + 1], Sc = k1 - k0;
    const size_t R0 = (size_t)off[k0], Rc = (size_t)off[k1] - R0, Qc = Rc + Sc;
    size_t o[6];
    stage_o(k0, k1, o);
    unsigned long long* h_off = reinterpret_cast<unsigned long long*>(f->h_ip);
    unsigned char* h_recs = f->h_ip + o[1];
    double* h_fco = reinterpret_cast<double*>(f->h_ip + o[2]);
    const FleetSeries* h_ser = reinterpret_cast<const FleetSeries*>(f->h_ip + o[3]);
    const double* h_out = reinterpret_cast<const double*>(f->h_ip + o[4]);
    for (uint32_t k = k0; k <= k1; ++k) h_off[k - k0] = off[k] - R0;
    fleet_parallel(Sc, 2 * Rc, [&](size_t lo, size_t hi) {
      for (size_t kl = lo; kl < hi; ++kl) {
        const size_t k = k0 + kl, a = (size_t)off[k], b = (size_t)off[k + 1];
        double* fco = h_fco + (a - R0 + kl) * (size_t)d;      // the series' first output row
        if (b == a) { std::fill(fco, fco + d, 0.0); continue; }
        double m = t[a];
        for (size_t s = a + 1; s < b; ++s) m = (t[s] < m) ? t[s] : m;      // data.minBy(_.t).t
        double tp = m;
        for (size_t s = a; s < b; ++s) {
          fleet_pack_rec(f->models[k], tp, t[s], y[s], has_obs ? (int)has_obs[s] : 1, (uint32_t)(s - a), h_recs + (s - R0) * RB);
          tp = t[s];
        }
        for (size_t q = 0; q <= b - a; ++q) {                  // F(time of output row q), as cssm_pf_interpolate's summaries build it
          const double time = q ? t[a + q - 1] : m;
          StepRec r;
          cssm_build_rec(&f->models[k], time, time, 0.0, 0, 0u, &r);
          for (int cc = 0; cc < d; ++cc) fco[q * (size_t)d + cc] = r.fco[cc];
        }
      }
    });
    if (Rc) {
      double* d_hist = reinterpret_cast<double*>(f->d_ip_hist);
      uint32_t* d_hanc = reinterpret_cast<uint32_t*>(f->d_ip_hist + Qc * (size_t)d * n * 8u);
      HIP_TRY(hipMemcpyAsync(f->d_ip, f->h_ip, o[3], hipMemcpyHostToDevice, f->stream));
      HIP_TRY(hipEventRecord(f->ev_ip[0], f->stream));
      FleetLaunch l;
      l.args.n = n; l.args.state = f->state; l.args.anc = f->anc; l.args.ser = f->ser; l.args.par = f->par;
      l.args.off = reinterpret_cast<const unsigned long long*>(f->d_ip);
      l.args.ctl = nullptr; l.args.recs = f->d_ip + o[1];
      l.args.ll_t = nullptr; l.args.ess_t = nullptr; l.args.logtab = f->logtab; l.args.mk = f->base.mk;
      l.args.picks = nullptr; l.args.path = nullptr; l.args.last = nullptr;
      l.args.fc = FleetOneStep{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
      l.args.hist = d_hist; l.args.hanc = d_hanc; l.args.hser = reinterpret_cast<FleetSeries*>(f->d_ip + o[3]); l.args.k0 = k0;
      l.n_series = Sc; l.path = false; l.hist = true; l.threads = f->threads; l.lds = f->lds; l.stream = f->stream;
      rc = fleet_series_launch(d, l);
      if (rc) return rc;
      HIP_TRY(hipEventRecord(f->ev_ip[1], f->stream));
      FleetLinLaunch q;
      q.args.n = n; q.args.np2 = np2; q.args.pairing = pairing ? 1u : 0u;
      q.args.hist = d_hist; q.args.hanc = d_hanc;
      q.args.off = l.args.off; q.args.ser = l.args.hser; q.args.recs = l.args.recs;
      q.args.fco = reinterpret_cast<const double*>(f->d_ip + o[2]);
      q.args.out = reinterpret_cast<double*>(f->d_ip + o[4]);
      q.args.mk = f->base.mk;
      q.args.lo_state = (uint32_t)rs.rank[0]; q.args.hi_state = (uint32_t)rs.rank[1];
      q.args.lo_eta = (uint32_t)re.rank[0]; q.args.hi_eta = (uint32_t)re.rank[1];
      q.d = d; q.n_series = Sc; q.stream = f->stream;
      const int hrc = cssm_fleet_lineage_launch(q);
      if (hrc) return fail(CSSM_EHIP, "k_fleet_lineage: %s", hipGetErrorString((hipError_t)hrc));
      HIP_TRY(hipEventRecord(f->ev_ip[2], f->stream));
      HIP_TRY(hipMemcpyAsync(f->h_ip + o[3], f->d_ip + o[3], o[5] - o[3], hipMemcpyDeviceToHost, f->stream));
      HIP_TRY(hipStreamSynchronize(f->stream));
      float m0 = 0.f, m1 = 0.f;
      if (hipEventElapsedTime(&m0, f->ev_ip[0], f->ev_ip[1]) == hipSuccess && hipEventElapsedTime(&m1, f->ev_ip[1], f->ev_ip[2]) == hipSuccess) {
        ms[0] += (double)m0; ms[1] += (double)m1;
      }
    }
    for (uint32_t kl = 0; kl < Sc; ++kl) {
      const uint32_t k = k0 + kl;
      const size_t a = (size_t)off[k], T = (size_t)off[k + 1] - a, lrow = a - R0 + kl, grow = a + k;
      if (T == 0) rc_out[k] = CSSM_EINVAL_ARG;                 // (the reference's minBy throws on an empty Vector)
      else rc_out[k] = h_ser[kl].err ? CSSM_ENONFINITE : CSSM_OK;
      const bool ok = rc_out[k] == CSSM_OK;
      ll_out[k] = ok ? h_ser[kl].ll : cssm_nan();
      for (size_t q = 0; q <= T; ++q) {
        const double* ho = h_out + (lrow + q) * (size_t)rows * 3u;
        double mean[CSSM_MAX_DIM];
        for (int cc = 0; cc < d; ++cc) {
          mean[cc] = ok ? ho[3 * cc] : cssm_nan();
          if (state_mean) state_mean[(grow + q) * d + cc] = mean[cc];
          if (state_lower) state_lower[(grow + q) * d + cc] = ok ? ho[3 * cc + 1] : cssm_nan();
          if (state_upper) state_upper[(grow + q) * d + cc] = ok ? ho[3 * cc + 2] : cssm_nan();
        }
        if (eta_lower) eta_lower[grow + q] = ok ? ho[3 * d + 1] : cssm_nan();
        if (eta_upper) eta_upper[grow + q] = ok ? ho[3 * d + 2] : cssm_nan();
        if (eta_of_mean) eta_of_mean[grow + q] = ok ? cssm_eta_of_mean(f->models[k], h_fco + (lrow + q) * (size_t)d, mean) : cssm_nan();   // :420
      }
    }
  }
  f->ms_ip[0] = ms[0]; f->ms_ip[1] = ms[1]; f->ip_ran = true;
  return CSSM_OK;
}

extern "C" int cssm_fleet_interpolate_last_ms(cssm_fleet* f, double* ms2) {
  if (!f || !ms2) return fail(CSSM_EINVAL_ARG, "null argument");
  if (!f->ip_ran) return fail(CSSM_ESTATE, "no interpolation has run on this fleet (cssm_fleet_interpolate first)");
  ms2[0] = f->ms_ip[0]; ms2[1] = f->ms_ip[1];
  return CSSM_OK;
}

extern "C" uint64_t cssm_fleet_observation_index(const cssm_fleet* f, uint32_t k) { return (f && k < f->S) ? f->step[k] : 0; }

extern "C" int cssm_fleet_get_particles(cssm_fleet* f, uint32_t k, double* out_dN) {
  if (!f || !out_dN) return fail(CSSM_EINVAL_ARG, "null argument");
  if (k >= f->S) return fail(CSSM_EINVAL_ARG, "series %u of %u", k, f->S);
  if (!f->live[k]) return fail(CSSM_ESTATE, "series %u has no cloud (not initialised, or its weights were unusable)", k);
  HIP_TRY(hipSetDevice(f->device));
  const uint32_t n = f->n;
  const double* src = f->state + ((size_t)k * 2u + (f->step[k] & 1u)) * f->d * n;
  hipLaunchKernelGGL(k_gather, dim3(grid_for(n, 256, 64)), dim3(256), 0, f->stream, src, (size_t)n, f->anc + (size_t)k * n, f->d_tmp, (size_t)n, (uint64_t)n,
                     f->d, (const double*)nullptr, (size_t)0, 0u);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(out_dN, f->d_tmp, (size_t)f->d * n * 8, hipMemcpyDeviceToHost, f->stream));
  HIP_TRY(hipStreamSynchronize(f->stream));
  return CSSM_OK;
}

extern "C" int cssm_fleet_get_ancestors(cssm_fleet* f, uint32_t k, uint32_t* out_N) {
  if (!f || !out_N) return fail(CSSM_EINVAL_ARG, "null argument");
  if (k >= f->S) return fail(CSSM_EINVAL_ARG, "series %u of %u", k, f->S);
  if (!f->live[k]) return fail(CSSM_ESTATE, "series %u has no cloud (not initialised, or its weights were unusable)", k);
  HIP_TRY(hipSetDevice(f->device));
  HIP_TRY(hipMemcpyAsync(out_N, f->anc + (size_t)k * f->n, (size_t)f->n * 4, hipMemcpyDeviceToHost, f->stream));
  HIP_TRY(hipStreamSynchronize(f->stream));
  return CSSM_OK;
}

extern "C" int cssm_fleet_last_ms(cssm_fleet* f, double* ms2) {
  if (!f || !ms2) return fail(CSSM_EINVAL_ARG, "null argument");
  ms2[0] = (double)f->ms_call; ms2[1] = (double)f->ms_summary; ms2[2] = (double)f->ms_forecast;
  return CSSM_OK;
}

// The compact record of one observation as the fleet uploads it (tests: its fields against cssm_build_rec's StepRec).  No device.
extern "C" int cssm_fleet_pack_record(const cssm_model_desc* desc, uint64_t n_particles, uint64_t seed, double t_prev, double t, double y,
                                      int has_obs, uint32_t step, unsigned char* out, size_t cap, size_t* bytes) {
  if (!out || !bytes) return fail(CSSM_EINVAL_ARG, "null argument");
  HostModel m;
  const int rc = cssm_build_model(&m, desc, false);
  if (rc) return rc;
  m.n_global = n_particles; m.seed = seed;
  *bytes = CSSM_FLEET_REC_BYTES(m.d);
  if (cap < *bytes) return fail(CSSM_EINVAL_ARG, "record of %zu bytes, room for %zu", *bytes, cap);
  fleet_pack_rec(m, t_prev, t, y, has_obs, step, out);
  return CSSM_OK;
}
