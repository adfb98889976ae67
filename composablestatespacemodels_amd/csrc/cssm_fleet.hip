// cssm_fleet.hip -- host side of the fleet filter (include/cssm_pf.h, "fleet of independent series"): S series of one model structure,
// N <= CSSM_FLEET_MAX_N particles each, parameters / Philox key / data / clock of its own per series, advanced by ONE launch whose
// blocks are the series (cssm_fleet.hip.h: k_fleet_series, one object per latent dimension).  Also k_fleet_summary (getIntervals of
// every series, one block per (series, row)).  A fleet call never degenerates into S single-handle runs: what the kernels do not
// serve is refused when the fleet is created or parameterised.
//
// Per-observation constants: the host builds every record with cssm_build_rec -- the function the single handle uses, so its bits by
// construction -- and uploads the compact form (FleetRecHead + 5 d doubles: 80 + 40 d bytes per observation, not sizeof(StepRec)).
// Records of different series are independent: large calls build them on a few host threads.
//
// An LGCP fleet (cssm_fleet_create_lgcp) is the same object with another record and another instantiation of k_fleet_series
// (cssm_fleet_lgcp.hip.h): every record is an event, built by cssm_build_rec under the series' model as for a handle, and where f depends
// on time the rows of cssm_build_fsub_table of every event of the launch travel behind the records in the same upload.  What it does
// not serve is refused at the top of the entry point.
//
// cssm_fleet_copy_series (EXTENSION; k_fleet_copy, cssm_fleet_copy.hip.h) copies whole series between the series of one fleet or from a
// second fleet: what SMC2's resampling and adoption need of a fleet whose series are parameter particles.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <thread>

#include "cssm_internal.h"
#include "cssm_kernels.hip.h"
#include "cssm_fleet.hip.h"
#include "cssm_fleet_copy.hip.h"
#include "cssm_fleet_forecast.hip.h"
#include "cssm_fleet_interp.hip.h"
#include "cssm_fleet_smooth.hip.h"
#include "cssm_fleet_if2.hip.h"
#include "cssm_fleet_pmmh.hip.h"
#include "cssm_fleet_pmmh_lgcp.hip.h"
#include "cssm_simulate.hip.h"
#include "cssm_simulate_plan.h"

static_assert(CSSM_FLEET_MAX_N <= 4096, "k_fleet_summary sorts at most 4096 keys in LDS; k_fleet_series holds 12 bytes per particle there");

// A grow-only allocation of the fleet, on the device or pinned on the host.  It frees itself with the fleet: cssm_fleet_destroy keeps no
// list of them.
struct FleetBuf {
  void* p = nullptr;
  size_t cap = 0;   // bytes
  const bool pinned;
  explicit FleetBuf(bool pinned_ = false) : pinned(pinned_) {}
  FleetBuf(const FleetBuf&) = delete;
  FleetBuf& operator=(const FleetBuf&) = delete;
  ~FleetBuf() { release(); }
  void release() {
    if (p) (void)(pinned ? hipHostFree(p) : hipFree(p));
    p = nullptr; cap = 0;
  }
  // room for `bytes` -- and (slack) a quarter more, for what grows a little from call to call; false: no memory, the buffer is empty
  bool reserve(size_t bytes, bool slack) {
    if (bytes <= cap) return true;
    release();
    const size_t want = slack ? bytes + bytes / 4 : bytes;
    if ((pinned ? hipHostMalloc(&p, want, hipHostMallocDefault) : hipMalloc(&p, want)) != hipSuccess) { p = nullptr; return false; }
    cap = want;
    return true;
  }
  template <class T> T* at(size_t byte = 0) const { return reinterpret_cast<T*>(static_cast<unsigned char*>(p) + byte); }
};
// ... the same view of any staged bytes (a layout struct names the offsets once; its host and device views are taken with this)
template <class T> static T* fleet_at(void* base, size_t byte) { return reinterpret_cast<T*>(static_cast<unsigned char*>(base) + byte); }
static size_t fleet_pad8(size_t bytes) { return (bytes + 7u) & ~(size_t)7u; }

enum FleetEvent {
  EV_CALL_BEGIN, EV_CALL_END,             // a series launch: init / filter / step call
  EV_SUMMARY_BEGIN, EV_SUMMARY_END,
  EV_FORECAST_BEGIN, EV_FORECAST_END,
  EV_PATH_UPLOADED, EV_PATH_KERNEL_END,   // a path launch's upload | kernel | read-back
  EV_COUNT
};

struct cssm_fleet {
  int device = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev[EV_COUNT] = {};
  uint32_t n = 0, S = 0;
  int d = 0, threads = 64;
  size_t lds = 0;
  bool lgcp = false;                    // made by cssm_fleet_create_lgcp: FilterLgcp's records and launch
  HostModel base;                       // the structure every series shares
  std::vector<HostModel> models;        // per series: parameters, key (HostModel::seed), n_global = n
  std::vector<double> t;                // per series: its clock
  std::vector<uint32_t> step;           // ... its observation index (Philox counter word; parity = the buffer that holds its cloud)
  std::vector<uint8_t> live;            // ... a cloud exists (initialised and not failed since)
  std::vector<int> obs_has_scale;       // ... the leftmost leaf's scale as stored (forecasts: cssm_obs_params_make)
  std::vector<double> obs_scale;
  bool par_dirty = true;
  // device, sized by cssm_fleet_create: double [S][2][d][n] | uint32 [S][n] | FleetSeries [S] | FleetPar [S] | the contract's table |
  // d x n doubles (cssm_fleet_get_particles)
  FleetBuf state, anc, ser, par, logtab, d_tmp;
  // grow-only, device and pinned host
  FleetBuf d_stage, h_stage{true};      // a series launch as staged (FleetStage) and its pinned mirror
  FleetBuf d_ll_t, d_ess_t;             // ... its per-observation results
  FleetBuf d_rows;                      // ... what its rider writes: sampled paths, filtered intervals or one-step-ahead forecasts (FleetStage)
  FleetBuf d_sm;                        // cssm_fleet_summary as staged (FleetSmStage)
  FleetBuf d_fc, h_fc{true};            // cssm_fleet_forecast / _forecast_posterior as staged (FleetFcStage) and its pinned mirror
  FleetBuf d_fc_scratch;                // [S][2][n]: eta and the observation draw of every forecast kernel (fleet_fc_scratch)
  FleetBuf d_fc_samp;                   // the samples of one chunk of series (at most fc_samp_max bytes: CSSM_OPT_FORECAST_CAP)
  FleetBuf d_ip, h_ip{true};            // one chunk of cssm_fleet_interpolate as staged (FleetIpStage) and its pinned mirror
  FleetBuf d_ip_hist;                   // ... its lineage history (clouds, then ancestors: at most ip_hist_max bytes, CSSM_OPT_INTERP_CAP)
  FleetBuf d_sim, h_sim{true};          // cssm_fleet_simulate as staged (FleetSimStage) and its pinned mirror
  FleetBuf d_sim_out, d_sim_carry;      // ... the rows of one chunk (at most fc_samp_max bytes, one time index at least); the states between
                                        //     the launches of a series that is run in windows of time indices
  float ms_simulate = -1.f;             // ... the device time of the last call (cssm_fleet_simulate_last_ms)
  std::vector<FleetSeries> h_ser;
  float ms_call = -1.f, ms_summary = -1.f, ms_forecast = -1.f;
  float ms_upload = -1.f, ms_kernel = -1.f;        // cssm_fleet_filter: ... of its last launch
  double ms_build = 0.0;                           // ... host time of its records
  double pm_split[6] = {0, 0, 0, 0, 0, 0};         // cssm_fleet_pmmh_run: see cssm_fleet_pmmh_last_split
  size_t fc_samp_max = (size_t)1 << 30;
  int fc_select = 0;                    // CSSM_OPT_FLEET_SELECT: 0 = by N (CSSM_FLEET_SELECT_MIN_N), 1 = bitonic sort, 2 = radix select
  size_t ip_hist_max = (size_t)1 << 30;
  hipEvent_t ev_ip[3] = {nullptr, nullptr, nullptr};   // before the forward launch | between the two | behind the lineage launch
  double ms_ip[2] = {-1.0, -1.0};                      // ... of the last interpolation, summed over its chunks
  bool ip_ran = false;
  FleetBuf d_bs_traj;                   // cssm_fleet_smooth: the trajectories of one chunk ([slices of the chunk][n_traj] uint32)
  hipEvent_t ev_bs = nullptr;           // ... behind its summary launch (ev_ip mark the forward launch and the backward simulation)
  double ms_bs[3] = {-1.0, -1.0, -1.0}; // ... forward, backward, summary of the last call, summed over its chunks
  bool bs_ran = false;
  int bs_staging = 0;                   // CSSM_OPT_SMOOTH_STAGING: 0 = the gathered means in LDS where they fit, 1 = never (through L2)
  double ms_if2 = -1.0;                 // cssm_fleet_if2: the device time of the last call's launches (cssm_fleet_if2_last_ms)
  double ms_pmmh_chains = -1.0;         // cssm_fleet_pmmh_chains: the device time of the last call's launches (cssm_fleet_pmmh_chains_last_ms)
  double ms_pmmh_lgcp = -1.0;           // cssm_fleet_pmmh_chains_lgcp: ... (cssm_fleet_pmmh_chains_lgcp_last_ms)
  // the window of cssm_fleet_step_interpolate: per series a ring of win_slices slots, each a cloud and the ancestors that resampled it
  // ([S][slices][d][n] doubles, then [S][slices][n] uint32).  Per series on the host: whether the window is continuous (the cloud the
  // fleet holds is the one its newest slot holds), the newest slot, the records remembered behind the base slice; per slot F at its time
  // and whether a weighted record wrote it.
  FleetBuf win;
  uint32_t win_slices = 0;
  std::vector<uint8_t> win_on, win_res;
  std::vector<uint32_t> win_head, win_depth;
  std::vector<double> win_fco;
  hipEvent_t ev_win[3] = {nullptr, nullptr, nullptr};   // before the forward launch | between the two | behind the lineage launch
  double ms_win[2] = {-1.0, -1.0};
  bool win_ran = false;
  FleetBuf d_copy;                      // cssm_fleet_copy_series within one fleet: the ancestors ([S][n] uint32) and scalars ([S] FleetSeries) between its two launches
  hipEvent_t ev_copy = nullptr;         // ... from a second fleet: recorded on the source's stream, waited for on this one
};
// series k's cloud, key or parameters are about to be written by another call than cssm_fleet_step_interpolate: its window restarts
static void fleet_win_drop(cssm_fleet* f, uint32_t k) {
  if (f->win_slices) { f->win_on[k] = 0; f->win_depth[k] = 0u; }
}
static void fleet_win_drop_all(cssm_fleet* f) {
  for (uint32_t k = 0; k < f->S && f->win_slices; ++k) fleet_win_drop(f, k);
}

#define FLEET_SERVED "cssm_pf_* (one handle per series) and cssm_pfb_* (batch of chains) serve it"
// what an LGCP fleet does not serve, said at the top of the entry point, before anything runs
#define FLEET_LGCP_REFUSE(f, call, served)                                                                                                    \
  if ((f) && (f)->lgcp)                                                                                                                       \
    return fail(CSSM_EINVAL_ARG, call ": an LGCP fleet filters event streams (cssm_fleet_ll_filter, _filter, _init, _step, _summary) and serves " \
                                      "nothing else yet; " served)
#define FLEET_LGCP_SERVED "cssm_pf_* (one handle per stream) serves it"

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

// (LGCP fleet) the compact record of the event at t behind t_prev: cssm_build_rec's, and the rows of cssm_build_fsub_table appended to `tab`
// -- the table of the caller's choice: fsub_off counts from `tab_base` doubles before it (where `tab` starts in the launch's table)
static int fleet_pack_rec_lgcp(const HostModel& m, double t_prev, double t, uint32_t step, unsigned char* dst, std::vector<double>& tab, size_t tab_base) {
  StepRec r;
  cssm_build_rec(&m, t_prev, t, 0.0, 1, step, &r);
  const int rc = cssm_build_fsub_table(&m, &r, 0, 1, tab);
  if (rc) return rc;
  FleetLgcpRecHead h;
  h.u = r.u; h.dt = r.dt; h.n_sub = r.n_sub; h.step = r.step; h.fsub_off = (uint32_t)(tab_base + r.fsub_off); h.pick = r.pick;
  memcpy(dst, &h, sizeof h);
  double* tail = reinterpret_cast<double*>(dst + sizeof h);
  for (int k = 0; k < m.d; ++k) for (int q = 0; q < 4; ++q) tail[4 * k + q] = r.coef[k][q];
  for (int k = 0; k < m.d; ++k) tail[4 * m.d + k] = r.fco[k];
  return CSSM_OK;
}
// ... and the doubles of the sub-step table that the events t[0 .. count) behind t_prev take: n_sub x d each, n_sub as cssm_build_rec
// counts it (0 for a model whose f does not depend on time: no table)
static size_t fleet_lgcp_rows(const HostModel& m, double t_prev, const double* t, size_t count) {
  if (!m.lgcp_tdep) return 0;
  size_t rows = 0;
  for (size_t s = 0; s < count; ++s) {
    StepRec r;
    cssm_build_rec(&m, t_prev, t[s], 0.0, 1, 0u, &r);
    if (r.n_sub > 0) rows += (size_t)r.n_sub;
    t_prev = t[s];
  }
  return rows * (size_t)m.d;
}
// the most a launch's table may hold: cssm_build_fsub_table's own bound for a handle's call
static int fleet_lgcp_table_fits(size_t doubles) {
  if (doubles <= ((size_t)1 << 27)) return CSSM_OK;
  return fail(CSSM_ENOMEM, "the sub-step table of a time-dependent LGCP fleet launch would exceed 1 GiB (%zu coefficients)", doubles);
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
  for (hipEvent_t e : f->ev) if (e) (void)hipEventDestroy(e);
  for (hipEvent_t e : f->ev_ip) if (e) (void)hipEventDestroy(e);
  if (f->ev_bs) (void)hipEventDestroy(f->ev_bs);
  for (hipEvent_t e : f->ev_win) if (e) (void)hipEventDestroy(e);
  if (f->ev_copy) (void)hipEventDestroy(f->ev_copy);
  if (f->stream) (void)hipStreamDestroy(f->stream);
  delete f;   // (every FleetBuf frees itself)
}

// cssm_fleet_create and cssm_fleet_create_lgcp: one body behind the question which observation model the call serves
static int fleet_create(const cssm_model_desc* desc, uint64_t n_particles, uint32_t n_series, int device, cssm_fleet** out, bool lgcp) {
  if (!out) return fail(CSSM_EINVAL_ARG, "out is null");
  *out = nullptr;
  if (n_particles < 1 || n_particles > CSSM_FLEET_MAX_N)
    return fail(CSSM_EINVAL_ARG, "a fleet holds 1 .. %d particles per series (a cloud lives in one workgroup's LDS), not %llu; " FLEET_SERVED,
                CSSM_FLEET_MAX_N, (unsigned long long)n_particles);
  if (n_series < 1) return fail(CSSM_EINVAL_ARG, "a fleet needs at least one series");
  HostModel base;
  int rc = cssm_build_model(&base, desc, false);
  if (rc) return rc;
  if (!lgcp && base.obs_kind == CSSM_OBS_LGCP)
    return fail(CSSM_EINVAL_DESC, "the fleet filter does not serve the LGCP observation model (sub-stepped events); " FLEET_SERVED);
  if (lgcp && base.obs_kind != CSSM_OBS_LGCP)
    return fail(CSSM_EINVAL_DESC, "cssm_fleet_create_lgcp makes a fleet of LGCP event streams (obs_kind %d given): cssm_fleet_create serves every other "
                                  "observation model", base.obs_kind);
  rc = cssm_use_device(device);
  if (rc) return rc;
  cssm_fleet* f = new cssm_fleet();
  f->device = device; f->n = (uint32_t)n_particles; f->S = n_series; f->d = base.d; f->lgcp = lgcp;
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
  if (hipEventCreate(&f->ev_bs) != hipSuccess) return bail(CSSM_EHIP, "hipEventCreate");
  for (hipEvent_t& e : f->ev_win) if (hipEventCreate(&e) != hipSuccess) return bail(CSSM_EHIP, "hipEventCreate");
  const size_t rows = (size_t)S * 2u * f->d * n;
  if (!f->state.reserve(rows * 8, false) || !f->anc.reserve((size_t)S * n * 4, false) || !f->ser.reserve((size_t)S * sizeof(FleetSeries), false) ||
      !f->par.reserve((size_t)S * sizeof(FleetPar), false) || !f->logtab.reserve(sizeof(CSSM_TAB), false) || !f->d_tmp.reserve((size_t)f->d * n * 8, false))
    return bail(CSSM_ENOMEM, "device memory (16 d N bytes of state per series)");
  if (hipMemcpyAsync(f->logtab.p, CSSM_TAB, sizeof(CSSM_TAB), hipMemcpyHostToDevice, f->stream) != hipSuccess ||
      hipMemsetAsync(f->ser.p, 0, (size_t)S * sizeof(FleetSeries), f->stream) != hipSuccess ||
      hipStreamSynchronize(f->stream) != hipSuccess)
    return bail(CSSM_EHIP, "uploading the contract's table");
  *out = f;
  return CSSM_OK;
}

extern "C" int cssm_fleet_create(const cssm_model_desc* desc, uint64_t n_particles, uint32_t n_series, int device, cssm_fleet** out) {
  return fleet_create(desc, n_particles, n_series, device, out, false);
}
// FilterLgcp(mod, resample, precision) for S event streams: the descriptor's lgcp_precision is part of the fleet's structure
extern "C" int cssm_fleet_create_lgcp(const cssm_model_desc* desc, uint64_t n_particles, uint32_t n_series, int device, cssm_fleet** out) {
  return fleet_create(desc, n_particles, n_series, device, out, true);
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
  if (option == CSSM_OPT_SMOOTH_STAGING) {   // cssm_fleet_smooth's backward simulation: where the gathered cloud of a time index is read from
    if (value < 0 || value > 1) return fail(CSSM_EINVAL_ARG, "CSSM_OPT_SMOOTH_STAGING is 0 (LDS where it fits) or 1 (never: through L2), not %d", value);
    f->bs_staging = value;
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
  fleet_win_drop_all(f);
  return CSSM_OK;
}

extern "C" int cssm_fleet_reseed(cssm_fleet* f, const uint64_t* seeds) {
  if (!f || !seeds) return fail(CSSM_EINVAL_ARG, "null argument");
  for (uint32_t k = 0; k < f->S; ++k) f->models[k].seed = seeds[k];
  f->par_dirty = true;
  fleet_win_drop_all(f);
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
  HIP_TRY(hipMemcpyAsync(f->par.p, hp.data(), (size_t)f->S * sizeof(FleetPar), hipMemcpyHostToDevice, f->stream));
  HIP_TRY(hipStreamSynchronize(f->stream));   // (hp is pageable and dies here)
  f->par_dirty = false;
  return CSSM_OK;
}

// The interval ranks of a cloud of n (a state row; the eta / observation rows, as cssm_pf_summary takes them) and the power of two
// >= max(n, 2) a row's sort in LDS pads to: what every kernel that summarises rows takes.
struct FleetRanks {
  FleetRowRanks rk;
  uint32_t np2;
};
static FleetRanks fleet_ranks(uint32_t n, double interval) {
  SelState rs, re;
  sel_ranks(rs, n, interval, true);
  sel_ranks(re, n, interval, false);
  FleetRanks r{FleetRowRanks{(uint32_t)rs.rank[0], (uint32_t)rs.rank[1], (uint32_t)re.rank[0], (uint32_t)re.rank[1]}, 2u};
  while (r.np2 < n) r.np2 <<= 1;
  return r;
}

// off[k + 1] >= off[k] of a ragged layout, refused in the words every entry point uses ...
static int fleet_off_step(const char* name, const uint64_t* off, uint32_t k) {
  if (off[k + 1] >= off[k]) return CSSM_OK;
  return fail(CSSM_EINVAL_ARG, "%s must be non-decreasing (%s[%u] = %llu > %s[%u] = %llu)", name, name, k, (unsigned long long)off[k], name, k + 1,
              (unsigned long long)off[k + 1]);
}
// ... and a whole layout of S series
static int fleet_off_check(const uint64_t* off, uint32_t S) {
  if (off[0] != 0) return fail(CSSM_EINVAL_ARG, "off[0] must be 0");
  for (uint32_t k = 0; k < S; ++k)
    if (const int rc = fleet_off_step("off", off, k)) return rc;
  return CSSM_OK;
}

// The caller's arrays of a call that returns getIntervals (cssm_fleet_summary, _interpolate, _filter_intervals, _step_intervals), and
// row `row` of them from a block's [d + 1][3] (mean, lower, upper of the d states and of eta).  Eta of the mean is formed here
// (model/ParticleFilter.scala:420) from the row's own f coefficients.  ok == false: the row reads NaN.
struct FleetIvOut {
  double *state_mean, *state_lower, *state_upper, *eta_of_mean, *eta_lower, *eta_upper;
};
static void fleet_iv_row(const cssm_fleet* f, uint32_t k, const double* src, const double* fco, bool ok, const FleetIvOut& o, size_t row) {
  const int d = f->d;
  auto at = [&](int r, int q) { return ok ? src[3 * r + q] : cssm_nan(); };
  double mean[CSSM_MAX_DIM];
  for (int c = 0; c < d; ++c) {
    mean[c] = at(c, 0);
    if (o.state_mean) o.state_mean[row * d + c] = mean[c];
    if (o.state_lower) o.state_lower[row * d + c] = at(c, 1);
    if (o.state_upper) o.state_upper[row * d + c] = at(c, 2);
  }
  if (o.eta_lower) o.eta_lower[row] = at(d, 1);
  if (o.eta_upper) o.eta_upper[row] = at(d, 2);
  if (o.eta_of_mean) o.eta_of_mean[row] = ok ? cssm_eta_of_mean(f->models[k], fco, mean) : cssm_nan();
}

// The caller's arrays of a call that returns forecasts (cssm_fleet_forecast, _forecast_posterior, _filter_forecasts, _step_forecast),
// and row `row` of them from a block's [d + 2][3] (mean, lower, upper of the d states, of eta and of the observation) and, where the
// call has them, its 2 PIT counts.  ok == false: the row reads NaN and -1.
struct FleetFcOut {
  double *state_mean, *state_lower, *state_upper, *eta_mean, *eta_lower, *eta_upper, *obs_mean, *obs_lower, *obs_upper;
  int32_t *obs_below, *obs_equal;
};
static void fleet_fc_row(int d, const double* src, const int32_t* pit, bool ok, const FleetFcOut& o, size_t row) {
  auto at = [&](int r, int q) { return ok ? src[3 * r + q] : cssm_nan(); };
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
  if (o.obs_below) o.obs_below[row] = ok ? pit[0] : -1;
  if (o.obs_equal) o.obs_equal[row] = ok ? pit[1] : -1;
}

// The layout of a series launch of R records, computed once per launch (fleet_ensure): every size and pointer of the launch, and what
// an entry point reads in the staging after the launch, derives from it.
// Staged, one upload: [S + 1 offsets (u64)] [S control words (u32), padded to 8 bytes] [R compact records] [the rider's:
//   path: R sampleOne slots (u32) | ival: [S][d] f coefficients, F at every series' t0 | fcst: R keys (u64), R data (f64), S observation
//   parameters, R flags (u32) padded to 8 bytes | ring: R slots (u32) and S base slots (u32), each padded to 8 bytes, then the lineage
//   launch's Q requests (FleetWinReq), Q x L slot words (u32, padded), Q x L x d f coefficients] -- a launch carries one rider at most.
// A launch that starts clouds from the caller's states (cssm_fleet_init_from; no records, no rider): [S + 1 row offsets (u64)] [S keys
// (u64)] [M rows of d doubles] [the caller's picks: S x N (u32), padded -- where given]; the rows taken come back in d_rows ([S][N] u32).
// An LGCP fleet's launch: the records are FleetLgcpRecHead ones, sampleOne's slots live inside them (no path rider is staged), and the
// launch's sub-step table (doubles; empty unless f depends on time) comes last.
// Written by the rider into d_rows, preset to 0xff bytes (NaN; -1 in the counts) for what no block writes:
//   path: [S][d] last rows, then (asked for) the R + S rows of the paths | ival: `rows` of [d + 1][3] | fcst: `rows` of [d + 2][3], then
//   `rows` of 2 PIT counts (i32) | ring: Q x L rows of [d + 1][3], written by the lineage launch.
static_assert(sizeof(cssm_obs_params) == 16, "the [S] array of observation parameters is uploaded as it is");
struct FleetStage {
  FleetKind kind = FleetKind::plain;
  bool lgcp = false;
  size_t R = 0, rec_bytes = 0;
  size_t fsub = 0, fsub_doubles = 0;                                                   // (LGCP fleet) the sub-step table
  size_t ctl = 0, recs = 0, ride = 0, fc_y = 0, fc_op = 0, fc_flags = 0, bytes = 0;   // byte offsets into the staging, and its size
  size_t w_base = 0, w_req = 0, w_words = 0, w_fco = 0;                                // ... of the ring rider
  bool from = false;                                                                   // cssm_fleet_init_from's launch ...
  size_t fr_keys = 0, fr_x = 0, fr_pick = 0;                                           // ... and its offsets (the row offsets are at `ride`)
  size_t rows = 0, out_doubles = 0, rows_bytes = 0;   // d_rows: the rows of ival / fcst and their doubles; the bytes of any rider
};
struct FleetStageView {   // the staging on the host or on the device; the pointers of another rider are null
  unsigned long long* off; uint32_t* ctl; unsigned char* recs;
  uint32_t* picks;
  double* fco0;
  unsigned long long* keys; double* y; cssm_obs_params* op; uint32_t* flags;
  uint32_t *w_slot, *w_base; FleetWinReq* w_req; uint32_t* w_words; double* w_fco;
  double* fsub;
  unsigned long long *fr_moff, *fr_keys; double* fr_x; uint32_t* fr_pick;
};
static FleetStageView fleet_view(const FleetStage& st, const FleetBuf& b) {
  FleetStageView v{};
  v.off = b.at<unsigned long long>(); v.ctl = b.at<uint32_t>(st.ctl); v.recs = b.at<unsigned char>(st.recs);
  if (st.kind == FleetKind::path && !st.lgcp) v.picks = b.at<uint32_t>(st.ride);
  if (st.lgcp) v.fsub = b.at<double>(st.fsub);
  if (st.from) {
    v.fr_moff = b.at<unsigned long long>(st.ride); v.fr_keys = b.at<unsigned long long>(st.fr_keys); v.fr_x = b.at<double>(st.fr_x);
    if (st.fr_pick) v.fr_pick = b.at<uint32_t>(st.fr_pick);
  }
  if (st.kind == FleetKind::ival) v.fco0 = b.at<double>(st.ride);
  if (st.kind == FleetKind::fcst) {
    v.keys = b.at<unsigned long long>(st.ride); v.y = b.at<double>(st.fc_y);
    v.op = b.at<cssm_obs_params>(st.fc_op); v.flags = b.at<uint32_t>(st.fc_flags);
  }
  if (st.kind == FleetKind::ring) {
    v.w_slot = b.at<uint32_t>(st.ride); v.w_base = b.at<uint32_t>(st.w_base); v.w_req = b.at<FleetWinReq>(st.w_req);
    v.w_words = b.at<uint32_t>(st.w_words); v.w_fco = b.at<double>(st.w_fco);
  }
  return v;
}
// the f coefficients of staged record r
static const double* fleet_rec_fco(const FleetStageView& v, int d, size_t r) {
  return reinterpret_cast<const double*>(v.recs + r * CSSM_FLEET_REC_BYTES(d) + sizeof(FleetRecHead)) + 4 * d;
}

// What rides behind the records of a series launch -- nothing (plain), `filter`'s sampled path, getIntervals of every cloud (ival), the
// forecast of every record before it is stepped (fcst), the window every record is remembered in and the lineage launch behind it
// (ring) -- with that rider's inputs and what it brings back.  (hist is cssm_fleet_interpolate's own launch: it stages chunk by chunk,
// FleetIpStage.)
struct FleetRide {
  FleetKind kind = FleetKind::plain;
  bool step = false;                 // ival / fcst: one row per series (cssm_fleet_step_*), not T_k + 1 / T_k rows per series
  bool more = false;                 // plain / ival: the records CONTINUE every series from the cloud it holds (cssm_fleet_*_more): none is drawn,
                                     // ival has a row per record and none for an initial cloud
  bool from = false;                 // plain, no records: cssm_fleet_init_from -- from_M rows in all, the caller's picks or none, the rows taken
  size_t from_M = 0;
  bool from_picks = false;
  uint32_t* pick_out = nullptr;
  double interval = 0.0;             // ival / fcst
  double *path_out = nullptr, *last_out = nullptr;   // path: receive the rows; either may be null
  const uint64_t* keys = nullptr;    // fcst: the caller's, one per record as the caller counts them ([off[S]], or [S] for a step), or null
  FleetIvOut ivo{};                  // ival, step: the caller's arrays (the entries of a series that is inactive, has no cloud or fails are not written)
  FleetFcOut fco{};                  // fcst, step: ...
  int* fc_rc_out = nullptr;
  const uint32_t* lag = nullptr;     // ring: the caller's [S], or null = max_lag for every series
  uint32_t max_lag = 0;
  uint32_t* rows_out = nullptr;
  size_t win_Q = 0, win_L = 0;       // ring: the series that ask for rows; the rows a request holds on the device (min(max_lag + 1, slices))
  FleetStage st;                     // the launch's layout (fleet_ensure)
  std::vector<double> out;           // ival / fcst: the rows as the device left them; NaN where no block wrote
  std::vector<int32_t> pit;          // fcst: ... -1 where no block wrote
  size_t fsub_doubles = 0;           // (LGCP fleet) the doubles of the launch's sub-step table, counted before the launch is laid out
  std::vector<int> fc_rc;            // fcst, [S]: the forecast's own status of every series
  std::string scale_msg;             // fcst: the reference's exception for the first series without the scale its observation needs
};

// lay a launch of R records with this rider out (ride.st) and make room for it: the staging, its pinned mirror, the per-observation results
static int fleet_ensure(cssm_fleet* f, size_t R, FleetRide& ride) {
  const size_t S = f->S, d = (size_t)f->d;
  FleetStage& st = ride.st;
  st = FleetStage();
  st.kind = ride.kind; st.R = R; st.lgcp = f->lgcp;
  st.rec_bytes = f->lgcp ? CSSM_FLEET_LGCP_REC_BYTES(f->d) : CSSM_FLEET_REC_BYTES(f->d);
  st.ctl = (S + 1u) * 8u;
  st.recs = st.ctl + fleet_pad8(S * 4u);
  st.ride = st.recs + R * st.rec_bytes;
  st.bytes = st.ride;
  if (st.kind == FleetKind::path) {
    if (!st.lgcp) st.bytes += R * 4u;
    st.rows_bytes = (S * d + (ride.path_out ? (R + S) * d : 0u)) * 8u;
  } else if (st.kind == FleetKind::ival) {
    st.bytes += S * d * 8u;
    st.rows = ride.step ? S : ride.more ? R : R + S;
    st.out_doubles = st.rows * (d + 1) * 3u;
    st.rows_bytes = st.out_doubles * 8u;
  } else if (st.kind == FleetKind::fcst) {
    st.fc_y = st.ride + R * 8u; st.fc_op = st.fc_y + R * 8u; st.fc_flags = st.fc_op + S * sizeof(cssm_obs_params);
    st.bytes = st.fc_flags + fleet_pad8(R * 4u);
    st.rows = ride.step ? S : R;
    st.out_doubles = st.rows * (d + 2) * 3u;
    st.rows_bytes = st.out_doubles * 8u + st.rows * 8u;
  } else if (st.kind == FleetKind::ring) {
    st.w_base = st.ride + fleet_pad8(R * 4u); st.w_req = st.w_base + fleet_pad8(S * 4u);
    st.w_words = st.w_req + ride.win_Q * sizeof(FleetWinReq); st.w_fco = st.w_words + fleet_pad8(ride.win_Q * ride.win_L * 4u);
    st.bytes = st.w_fco + ride.win_Q * ride.win_L * d * 8u;
    st.rows = ride.win_Q * ride.win_L;
    st.out_doubles = st.rows * (d + 1) * 3u;
    st.rows_bytes = st.out_doubles * 8u;
  }
  if (ride.from) {
    st.from = true;
    st.fr_keys = st.ride + (S + 1u) * 8u; st.fr_x = st.fr_keys + S * 8u;
    st.bytes = st.fr_x + ride.from_M * d * 8u;
    if (ride.from_picks) { st.fr_pick = st.bytes; st.bytes += fleet_pad8(S * f->n * 4u); }
    st.rows_bytes = ride.pick_out ? S * f->n * 4u : 0u;
  }
  if (st.lgcp) { st.fsub = fleet_pad8(st.bytes); st.fsub_doubles = ride.fsub_doubles; st.bytes = st.fsub + st.fsub_doubles * 8u; }
  if (!f->h_stage.reserve(st.bytes, true)) return fail(CSSM_ENOMEM, "fleet: %zu bytes of pinned staging", st.bytes);
  if (!f->d_stage.reserve(st.bytes, true)) return fail(CSSM_ENOMEM, "fleet: %zu bytes of records", st.bytes);
  const size_t rr = std::max<size_t>(R, 1);
  if (!f->d_ll_t.reserve(rr * 8, true) || !f->d_ess_t.reserve(rr * 4, true)) return fail(CSSM_ENOMEM, "fleet: per-observation results");
  return CSSM_OK;
}

// 16 N bytes of eta / obs staging per series: the scratch of every kernel that forecasts, allocated once
static int fleet_fc_scratch(cssm_fleet* f) {
  if (!f->d_fc_scratch.reserve((size_t)f->S * 2u * f->n * 8u, false)) return fail(CSSM_ENOMEM, "fleet forecast: 16 N bytes of staging per series");
  return CSSM_OK;
}

// what every launch of k_fleet_series takes from the fleet
static void fleet_series_args(const cssm_fleet* f, FleetLaunch& l) {
  l.args.n = f->n; l.args.state = f->state.at<double>(); l.args.anc = f->anc.at<uint32_t>();
  l.args.ser = f->ser.at<FleetSeries>(); l.args.par = f->par.at<FleetPar>();
  l.args.logtab = f->logtab.at<double>(); l.args.mk = f->base.mk;
  l.threads = f->threads; l.lds = f->lds; l.stream = f->stream;
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

// upload the staged launch (fleet_ensure laid it out, the caller filled it), run it with its rider, bring the series' scalars, the
// rider's rows and (asked for) the per-observation results back; synchronises.
static int fleet_launch(cssm_fleet* f, FleetRide& ride, double* ll_t, int32_t* ess_t) {
  int rc = fleet_upload_par(f);
  if (rc) return rc;
  const FleetStage& st = ride.st;
  const size_t R = st.R, n_last = (size_t)f->S * f->d;
  const bool path = st.kind == FleetKind::path, ival = st.kind == FleetKind::ival, fcst = st.kind == FleetKind::fcst, ring = st.kind == FleetKind::ring;
  if (!f->d_rows.reserve(st.rows_bytes, true))
    return fail(CSSM_ENOMEM, "fleet: %zu bytes of %s", st.rows_bytes,
                path ? "sampled paths" : ival ? "filtered intervals" : ring ? "fixed-lag rows" : st.from ? "picks" : "one-step-ahead forecasts");
  if (!ring) {   // the cloud of every series this launch runs is written outside its window
    const FleetStageView hv = fleet_view(st, f->h_stage);
    for (uint32_t k = 0; k < f->S; ++k)
      if (hv.off[k + 1] > hv.off[k] || (hv.ctl[k] & CSSM_FLEET_CTL_INIT)) fleet_win_drop(f, k);
  }
  if (fcst && (rc = fleet_fc_scratch(f))) return rc;
  HIP_TRY(hipEventRecord(f->ev[EV_CALL_BEGIN], f->stream));
  HIP_TRY(hipMemcpyAsync(f->d_stage.p, f->h_stage.p, st.bytes, hipMemcpyHostToDevice, f->stream));
  if (R) {   // records a failed series never reaches read as NaN / -1
    HIP_TRY(hipMemsetAsync(f->d_ll_t.p, 0xff, R * 8, f->stream));
    HIP_TRY(hipMemsetAsync(f->d_ess_t.p, 0xff, R * 4, f->stream));
  }
  if (st.rows_bytes) HIP_TRY(hipMemsetAsync(f->d_rows.p, 0xff, st.rows_bytes, f->stream));   // ... and the rows it never records, summarises or forecasts
  if (path) HIP_TRY(hipEventRecord(f->ev[EV_PATH_UPLOADED], f->stream));
  const FleetStageView dv = fleet_view(st, f->d_stage);
  double* rows = f->d_rows.at<double>();
  FleetLaunch l{};
  fleet_series_args(f, l);
  l.args.off = dv.off; l.args.ctl = dv.ctl; l.args.recs = dv.recs;
  l.args.ll_t = f->d_ll_t.at<double>(); l.args.ess_t = f->d_ess_t.at<int32_t>();
  l.n_series = f->S; l.kind = st.kind; l.lgcp = f->lgcp;
  if (f->lgcp && f->base.lgcp_tdep) l.args.fsub = dv.fsub;   // (otherwise null: f is every record's own)
  if (path) {
    l.args.picks = dv.picks; l.args.last = rows;
    if (ride.path_out) l.args.path = rows + n_last;
  }
  if (ival || fcst) {
    const FleetRanks r = fleet_ranks(f->n, ride.interval);
    l.args.iv_rows = ride.step ? 1u : ride.more ? 2u : 0u; l.args.iv_np2 = r.np2; l.args.iv_rk = r.rk;
    l.lds = (size_t)r.np2 * 8u + (size_t)f->n * 4u;   // the keys of a row's sort take the weights' place
    ride.out.resize(st.out_doubles);
  }
  if (ival) { l.args.iv_fco0 = dv.fco0; l.args.iv_out = rows; }
  if (fcst) {
    l.args.fc.keys = dv.keys; l.args.fc.y = dv.y; l.args.fc.op = dv.op; l.args.fc.flags = dv.flags;
    l.args.fc.stage = f->d_fc_scratch.at<double>();
    l.args.fc.out = rows; l.args.fc.pit = f->d_rows.at<int32_t>(st.out_doubles * 8u);
    ride.pit.resize(st.rows * 2u);
  }
  if (st.from) {
    l.args.fr_moff = dv.fr_moff; l.args.fr_keys = dv.fr_keys; l.args.fr_x = dv.fr_x; l.args.fr_pick = dv.fr_pick;
    if (ride.pick_out) l.args.fr_pick_out = f->d_rows.at<uint32_t>();
  }
  if (ring) {
    l.args.ring.x = f->win.at<double>(); l.args.ring.a = f->win.at<uint32_t>((size_t)f->S * f->win_slices * f->d * f->n * 8u);
    l.args.ring.slot = dv.w_slot; l.args.ring.base = dv.w_base; l.args.ring.slices = f->win_slices;
    ride.out.resize(st.out_doubles);
    HIP_TRY(hipEventRecord(f->ev_win[0], f->stream));
  }
  rc = fleet_series_launch(f->d, l);
  if (rc) return rc;
  if (ring) {   // the lineage launch: every block reads only what the forward launch finished
    HIP_TRY(hipEventRecord(f->ev_win[1], f->stream));
    if (ride.win_Q) {
      const FleetRanks r = fleet_ranks(f->n, ride.interval);
      FleetWinLaunch q;
      q.args.n = f->n; q.args.np2 = r.np2; q.args.slices = f->win_slices; q.args.L = (uint32_t)ride.win_L;
      q.args.ring_x = l.args.ring.x; q.args.ring_a = l.args.ring.a;
      q.args.req = dv.w_req; q.args.words = dv.w_words; q.args.ser = l.args.ser; q.args.fco = dv.w_fco; q.args.out = rows;
      q.args.mk = f->base.mk;
      q.args.lo_state = r.rk.lo_state; q.args.hi_state = r.rk.hi_state; q.args.lo_eta = r.rk.lo_eta; q.args.hi_eta = r.rk.hi_eta;
      q.d = f->d; q.n_req = (uint32_t)ride.win_Q; q.stream = f->stream;
      const int hrc = cssm_fleet_window_launch(q);
      if (hrc) return fail(CSSM_EHIP, "k_fleet_window: %s", hipGetErrorString((hipError_t)hrc));
      HIP_TRY(hipEventRecord(f->ev_win[2], f->stream));
    }
  }
  if (path) HIP_TRY(hipEventRecord(f->ev[EV_PATH_KERNEL_END], f->stream));
  HIP_TRY(hipMemcpyAsync(f->h_ser.data(), f->ser.p, (size_t)f->S * sizeof(FleetSeries), hipMemcpyDeviceToHost, f->stream));
  if (path && ride.path_out) HIP_TRY(hipMemcpyAsync(ride.path_out, rows + n_last, st.rows_bytes - n_last * 8, hipMemcpyDeviceToHost, f->stream));
  if (path && ride.last_out) HIP_TRY(hipMemcpyAsync(ride.last_out, rows, n_last * 8, hipMemcpyDeviceToHost, f->stream));
  if (R && ll_t) HIP_TRY(hipMemcpyAsync(ll_t, f->d_ll_t.p, R * 8, hipMemcpyDeviceToHost, f->stream));
  if (R && ess_t) HIP_TRY(hipMemcpyAsync(ess_t, f->d_ess_t.p, R * 4, hipMemcpyDeviceToHost, f->stream));
  if (st.out_doubles) HIP_TRY(hipMemcpyAsync(ride.out.data(), rows, st.out_doubles * 8u, hipMemcpyDeviceToHost, f->stream));
  if (st.from && ride.pick_out) HIP_TRY(hipMemcpyAsync(ride.pick_out, f->d_rows.p, st.rows_bytes, hipMemcpyDeviceToHost, f->stream));
  if (fcst && st.rows) HIP_TRY(hipMemcpyAsync(ride.pit.data(), l.args.fc.pit, st.rows * 8u, hipMemcpyDeviceToHost, f->stream));
  HIP_TRY(hipEventRecord(f->ev[EV_CALL_END], f->stream));
  HIP_TRY(hipStreamSynchronize(f->stream));
  if (hipEventElapsedTime(&f->ms_call, f->ev[EV_CALL_BEGIN], f->ev[EV_CALL_END]) != hipSuccess) f->ms_call = -1.f;
  if (path) {
    if (hipEventElapsedTime(&f->ms_upload, f->ev[EV_CALL_BEGIN], f->ev[EV_PATH_UPLOADED]) != hipSuccess) f->ms_upload = -1.f;
    if (hipEventElapsedTime(&f->ms_kernel, f->ev[EV_PATH_UPLOADED], f->ev[EV_PATH_KERNEL_END]) != hipSuccess) f->ms_kernel = -1.f;
  }
  if (ring) {
    float m0 = -1.f, m1 = 0.f;
    if (hipEventElapsedTime(&m0, f->ev_win[0], f->ev_win[1]) != hipSuccess) m0 = -1.f;
    if (ride.win_Q && hipEventElapsedTime(&m1, f->ev_win[1], f->ev_win[2]) != hipSuccess) m1 = -1.f;
    f->ms_win[0] = (double)m0; f->ms_win[1] = (double)m1; f->win_ran = true;
  }
  return CSSM_OK;
}

// fcst: the forecast's own status and the observation parameters of every series (runs(k): the launch has a record of series k).  The
// reference's exception is one message: formed in order.
template <class Runs>
static void fleet_fc_series(const cssm_fleet* f, FleetRide& ride, const FleetStageView& h, Runs runs) {
  ride.fc_rc.assign(f->S, CSSM_OK);
  for (uint32_t k = 0; k < f->S; ++k) {
    memset(&h.op[k], 0, sizeof(cssm_obs_params));
    if (runs(k) && cssm_obs_params_or_fail(f->base.obs_kind, f->obs_has_scale[k], f->obs_scale[k], f->base.obs_df, &h.op[k])) {
      if (ride.scale_msg.empty()) ride.scale_msg = "series " + std::to_string(k) + ": " + cssm_last_error();
      ride.fc_rc[k] = CSSM_EINVAL_ARG;
    }
  }
  if (ride.st.R & 1u) h.flags[ride.st.R] = 0u;   // (the padding travels too)
}
// fcst: the forecast of staged record r -- series k's observation `idx`, the caller's `slot` -- before it is stepped from t_prev to t:
// cssm_fleet_forecast's own refusals of a time, the key, the datum as given
static void fleet_fc_record(const cssm_fleet* f, const FleetRide& ride, const FleetStageView& h, uint32_t k, size_t r, size_t slot, uint32_t idx,
                            double t_prev, double t, double y, int has) {
  const bool on = ride.fc_rc[k] == CSSM_OK && std::isfinite(t) && t >= t_prev;
  h.flags[r] = on ? (CSSM_FLEET_FC_ON | (has ? CSSM_FLEET_FC_HAS : 0u)) : 0u;
  h.keys[r] = ride.keys ? ride.keys[slot] : cssm_pf_run_key(f->models[k].seed, (1ull << 63) | (uint64_t)idx);
  h.y[r] = y;
}

// llFilter / filter of every series: the records of all of them built (threaded above 8192), ONE upload, ONE launch with the call's
// rider, ONE read-back.  ride.more: the records continue every series from the cloud it holds (cssm_fleet_ll_filter_more) -- no cloud is
// drawn, a series' first increment is taken from its clock and its records count on from its observation index, as cssm_fleet_step's one
// record does; a series without a cloud gets no block, so the launch's records are the caller's without that series' (roff below).
static int fleet_filter_all(cssm_fleet* f, const uint64_t* off, const double* t, const double* y, const uint8_t* has_obs, double* ll_out, double* ll_t,
                            int32_t* ess_t, int* rc_out, FleetRide& ride) {
  const uint32_t S = f->S;
  const bool more = ride.more;
  int rc = fleet_off_check(off, S);
  if (rc) return rc;
  if (off[S] && (!t || (!y && !f->lgcp))) return fail(CSSM_EINVAL_ARG, "null data");
  if (more) {
    bool any_live = false;
    for (uint32_t k = 0; k < S; ++k) any_live = any_live || f->live[k];
    if (!any_live) return fail(CSSM_ESTATE, "no series of the fleet is initialised (cssm_fleet_init / cssm_fleet_ll_filter first)");
  }
  HIP_TRY(hipSetDevice(f->device));
  const auto tb0 = std::chrono::steady_clock::now();
  ride.step = false;
  auto runs = [&](size_t k) { return off[k + 1] > off[k] && (!more || f->live[k]); };
  std::vector<size_t> roff((size_t)S + 1u, 0);   // series k's records as the launch counts them: the caller's, unless a series is left out
  for (uint32_t k = 0; k < S; ++k) roff[k + 1] = roff[k] + (runs(k) ? (size_t)(off[k + 1] - off[k]) : 0u);
  const size_t R = roff[S];
  auto t_min = [&](size_t a, size_t b) {                                   // data.minBy(_.t).t
    double m = t[a];
    for (size_t s = a + 1; s < b; ++s) m = (t[s] < m) ? t[s] : m;
    return m;
  };
  auto t_start = [&](size_t k) { return more ? f->t[k] : t_min((size_t)off[k], (size_t)off[k + 1]); };   // where a series' first increment starts
  std::vector<size_t> toff;   // (LGCP fleet, f depends on time) where series k's rows start in the launch's sub-step table (doubles)
  if (f->lgcp && f->base.lgcp_tdep) {
    toff.assign((size_t)S + 1u, 0);
    fleet_parallel(S, R, [&](size_t lo, size_t hi) {
      for (size_t k = lo; k < hi; ++k) {
        const size_t a = (size_t)off[k], b = (size_t)off[k + 1];
        if (runs(k)) toff[k + 1] = fleet_lgcp_rows(f->models[k], t_start(k), t + a, b - a);
      }
    });
    for (uint32_t k = 0; k < S; ++k) toff[k + 1] += toff[k];
    if ((rc = fleet_lgcp_table_fits(toff[S]))) return rc;
    ride.fsub_doubles = toff[S];
  }
  rc = fleet_ensure(f, R, ride);
  if (rc) return rc;
  const FleetStageView h = fleet_view(ride.st, f->h_stage);
  const size_t RB = ride.st.rec_bytes;
  const bool fcst = ride.kind == FleetKind::fcst;
  if (fcst) fleet_fc_series(f, ride, h, [&](uint32_t k) { return off[k + 1] > off[k]; });
  for (uint32_t k = 0; k <= S; ++k) h.off[k] = roff[k];
  std::atomic<int> pack_rc{CSSM_OK};
  fleet_parallel(S, R, [&](size_t lo, size_t hi) {
    for (size_t k = lo; k < hi; ++k) {
      const size_t a = (size_t)off[k], b = (size_t)off[k + 1], r0 = roff[k];
      h.ctl[k] = (b > a && !more) ? CSSM_FLEET_CTL_INIT : 0u;
      if (h.fco0) for (int c = 0; c < f->d; ++c) h.fco0[k * f->d + c] = 0.0;   // (a launch that continues draws no cloud: not read)
      if (!runs(k)) continue;
      const double m = t_start(k);
      const uint32_t i0 = more ? f->step[k] : 0u;                        // the series' observation index at its first record
      if (f->lgcp) {                                                     // every record an event; the series' rows of the table behind them
        std::vector<double> tab;
        double tp = m;
        for (size_t s = a; s < b; ++s) {
          const int prc = fleet_pack_rec_lgcp(f->models[k], tp, t[s], i0 + (uint32_t)(s - a), h.recs + (r0 + s - a) * RB, tab, toff.empty() ? 0u : toff[k]);
          if (prc) pack_rc = prc;
          tp = t[s];
        }
        if (!tab.empty() && tab.size() == toff[k + 1] - toff[k]) memcpy(h.fsub + toff[k], tab.data(), tab.size() * 8u);
        else if (!tab.empty()) pack_rc = CSSM_ENOMEM;
        continue;
      }
      if (h.fco0 && !more) {                                             // F(t0): t0 need not be the first record's time
        StepRec rec0;
        cssm_build_rec(&f->models[k], m, m, 0.0, 0, 0u, &rec0);
        for (int c = 0; c < f->d; ++c) h.fco0[k * f->d + c] = rec0.fco[c];
      }
      double tp = m;
      for (size_t s = a; s < b; ++s) {
        const int has = has_obs ? (int)has_obs[s] : 1;
        const size_t r = r0 + (s - a);
        fleet_pack_rec(f->models[k], tp, t[s], y[s], has, i0 + (uint32_t)(s - a), h.recs + r * RB, h.picks ? h.picks + r : nullptr);
        if (fcst) fleet_fc_record(f, ride, h, (uint32_t)k, r, s, (uint32_t)(s - a), tp, t[s], y[s], has);
        tp = t[s];
      }
    }
  });
  if (pack_rc) return fail(pack_rc, "fleet: the sub-step table of the launch could not be built");
  if (ride.kind == FleetKind::path) f->ms_build = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tb0).count();
  // per-observation results: straight into the caller's arrays, unless a series was left out -- then by way of the launch's own order
  const bool same = R == (size_t)off[S];
  std::vector<double> r_ll(same || !ll_t ? 0u : R);
  std::vector<int32_t> r_ess(same || !ess_t ? 0u : R);
  rc = fleet_launch(f, ride, same ? ll_t : (ll_t ? r_ll.data() : nullptr), same ? ess_t : (ess_t ? r_ess.data() : nullptr));
  if (rc) return rc;
  for (uint32_t k = 0; k < S; ++k) {
    const size_t a = (size_t)off[k], b = (size_t)off[k + 1];
    if (!same) {
      for (size_t s = a; s < b; ++s) {
        if (ll_t) ll_t[s] = runs(k) ? r_ll[roff[k] + s - a] : cssm_nan();
        if (ess_t) ess_t[s] = runs(k) ? r_ess[roff[k] + s - a] : -1;
      }
    }
    if (more && b == a) { rc_out[k] = CSSM_OK; continue; }                 // continued by nothing: untouched
    if (more && !f->live[k]) { rc_out[k] = CSSM_ESTATE; continue; }        // no cloud: never initialised, or failed since
    if (b == a) { rc_out[k] = CSSM_EINVAL_ARG; ll_out[k] = cssm_nan(); continue; }   // (the reference's minBy throws on an empty Vector)
    const FleetSeries& s = f->h_ser[k];
    if (s.err) {
      rc_out[k] = CSSM_ENONFINITE; ll_out[k] = cssm_nan(); f->live[k] = 0;
    } else {
      rc_out[k] = CSSM_OK; ll_out[k] = s.ll; f->live[k] = 1; f->t[k] = t[b - 1]; f->step[k] = (more ? f->step[k] : 0u) + (uint32_t)(b - a);
    }
  }
  return CSSM_OK;
}

extern "C" int cssm_fleet_ll_filter(cssm_fleet* f, const uint64_t* off, const double* t, const double* y, const uint8_t* has_obs,
                                    double* ll_out, double* ll_t, int32_t* ess_t, int* rc_out) {
  if (!f || !off || !ll_out || !rc_out) return fail(CSSM_EINVAL_ARG, "null argument");
  FleetRide ride;
  return fleet_filter_all(f, off, t, y, has_obs, ll_out, ll_t, ess_t, rc_out, ride);
}

// filter (model/ParticleFilter.scala:152-158) of every series: cssm_fleet_ll_filter, and one particle of the initial cloud and of the
// cloud after every record (Resampling.sampleOne): the sampleOne slots travel behind the records.  What needs no fleet is refused first,
// so that it is refused on any host.
extern "C" int cssm_fleet_filter(cssm_fleet* f, const uint64_t* off, const double* t, const double* y, const uint8_t* has_obs, double* ll_out,
                                 double* ll_t, int32_t* ess_t, double* path_out, double* last_out, int* rc_out) {
  if (!off) return fail(CSSM_EINVAL_ARG, "off is null");
  if (!ll_out || !rc_out) return fail(CSSM_EINVAL_ARG, "ll_out / rc_out is null");
  if (!path_out && !last_out)
    return fail(CSSM_EINVAL_ARG, "neither path_out nor last_out is given: cssm_fleet_ll_filter is the call that records no path");
  if (off[0] != 0) return fail(CSSM_EINVAL_ARG, "off[0] must be 0");
  if (!t || (!y && !(f && f->lgcp))) return fail(CSSM_EINVAL_ARG, "null data");
  if (!f) return fail(CSSM_EINVAL_ARG, "null fleet");
  FleetRide ride;
  ride.kind = FleetKind::path; ride.path_out = path_out; ride.last_out = last_out;
  return fleet_filter_all(f, off, t, y, has_obs, ll_out, ll_t, ess_t, rc_out, ride);
}

// examples/Filtering.scala:24-31 of every series: cssm_fleet_ll_filter, and getIntervals (model/ParticleFilter.scala:415-424) of the initial
// cloud and of the cloud after every record, written by the series' own workgroup inside the one launch.  What needs no fleet is refused
// first, so that it is refused on any host.
extern "C" int cssm_fleet_filter_intervals(cssm_fleet* f, const uint64_t* off, const double* t, const double* y, const uint8_t* has_obs, double interval,
                                           double* ll_out, double* ll_t, int32_t* ess_t, double* state_mean, double* state_lower, double* state_upper,
                                           double* eta_of_mean, double* eta_lower, double* eta_upper, int* rc_out) {
  FLEET_LGCP_REFUSE(f, "cssm_fleet_filter_intervals", FLEET_LGCP_SERVED);
  if (!off) return fail(CSSM_EINVAL_ARG, "off is null");
  if (!ll_out || !rc_out) return fail(CSSM_EINVAL_ARG, "ll_out / rc_out is null");
  if (off[0] != 0) return fail(CSSM_EINVAL_ARG, "off[0] must be 0");
  if (!t || !y) return fail(CSSM_EINVAL_ARG, "null data");
  if (!(interval > 0.0 && interval <= 1.0)) return fail(CSSM_EINVAL_ARG, "interval must be in (0, 1]");
  if (!f) return fail(CSSM_EINVAL_ARG, "null fleet");
  FleetRide ride;
  ride.kind = FleetKind::ival; ride.interval = interval;
  int rc = fleet_filter_all(f, off, t, y, has_obs, ll_out, ll_t, ess_t, rc_out, ride);
  if (rc) return rc;
  const uint32_t S = f->S;
  const int d = f->d;
  const size_t R = ride.st.R, rowsz = (size_t)(d + 1) * 3u;
  const FleetIvOut o{state_mean, state_lower, state_upper, eta_of_mean, eta_lower, eta_upper};
  for (double* p : {state_mean, state_lower, state_upper}) if (p) std::fill(p, p + (R + S) * (size_t)d, cssm_nan());
  for (double* p : {eta_of_mean, eta_lower, eta_upper}) if (p) std::fill(p, p + (R + S), cssm_nan());
  const FleetStageView h = fleet_view(ride.st, f->h_stage);   // (the staged launch is still there: the f coefficients of every row)
  fleet_parallel(S, R, [&](size_t lo, size_t hi) {
    for (size_t k = lo; k < hi; ++k) {
      const size_t a = (size_t)off[k], b = (size_t)off[k + 1];
      if (b == a) continue;                                         // no records: NaN in its single row
      const FleetSeries& s = f->h_ser[k];
      const size_t nrows = s.err ? (size_t)s.fail_rec + 1u : b - a + 1u;   // a failure at observation s keeps rows 0 .. s
      for (size_t i = 0; i < nrows; ++i)
        fleet_iv_row(f, (uint32_t)k, ride.out.data() + (a + k + i) * rowsz, i ? fleet_rec_fco(h, d, a + i - 1) : h.fco0 + k * d, true, o, a + k + i);
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
  FLEET_LGCP_REFUSE(f, "cssm_fleet_filter_forecasts", FLEET_LGCP_SERVED);
  if (!off) return fail(CSSM_EINVAL_ARG, "off is null");
  if (!ll_out || !rc_out || !fc_rc_out) return fail(CSSM_EINVAL_ARG, "ll_out / rc_out / fc_rc_out is null");
  if (off[0] != 0) return fail(CSSM_EINVAL_ARG, "off[0] must be 0");
  if (!t || !y) return fail(CSSM_EINVAL_ARG, "null data");
  if (!(interval > 0.0 && interval <= 1.0)) return fail(CSSM_EINVAL_ARG, "interval must be in (0, 1]");
  if (!f) return fail(CSSM_EINVAL_ARG, "null fleet");
  FleetRide ride;
  ride.kind = FleetKind::fcst; ride.interval = interval; ride.keys = keys;
  int rc = fleet_filter_all(f, off, t, y, has_obs, ll_out, ll_t, ess_t, rc_out, ride);
  if (rc) return rc;
  const uint32_t S = f->S;
  const size_t rowsz = (size_t)(f->d + 2) * 3u;
  const FleetFcOut o{state_mean, state_lower, state_upper, eta_mean, eta_lower, eta_upper, obs_mean, obs_lower, obs_upper, obs_below, obs_equal};
  const FleetStageView h = fleet_view(ride.st, f->h_stage);   // (the staged launch is still there: the records' flags)
  fleet_parallel(S, ride.st.R, [&](size_t lo, size_t hi) {
    for (size_t k = lo; k < hi; ++k) {
      const size_t a = (size_t)off[k], b = (size_t)off[k + 1];
      fc_rc_out[k] = ride.fc_rc[k];
      const FleetSeries& s = f->h_ser[k];
      const size_t nrows = (b > a && s.err) ? (size_t)s.fail_rec + 1u : b - a;   // a failure at observation s keeps rows 0 .. s
      for (size_t r = a; r < b; ++r)
        fleet_fc_row(f->d, ride.out.data() + r * rowsz, ride.pit.data() + 2 * r, r - a < nrows && (h.flags[r] & CSSM_FLEET_FC_ON), o, r);
    }
  });
  if (!ride.scale_msg.empty()) (void)fail(CSSM_EINVAL_ARG, "%s", ride.scale_msg.c_str());   // (the call succeeds; the message names the first such series)
  return CSSM_OK;
}

// cssm_pf_ll_filter_more of every series: T_k MORE records of the filters that are already running, in the ONE launch of
// cssm_fleet_ll_filter -- fleet_filter_all in its continue mode.  What needs no fleet is refused first, so that it is refused on any host.
extern "C" int cssm_fleet_ll_filter_more(cssm_fleet* f, const uint64_t* off, const double* t, const double* y, const uint8_t* has_obs,
                                         double* ll_out, double* ll_t, int32_t* ess_t, int* rc_out) {
  if (!off) return fail(CSSM_EINVAL_ARG, "off is null");
  if (!ll_out || !rc_out) return fail(CSSM_EINVAL_ARG, "ll_out / rc_out is null");
  if (off[0] != 0) return fail(CSSM_EINVAL_ARG, "off[0] must be 0");
  if (!t || (!y && !(f && f->lgcp))) return fail(CSSM_EINVAL_ARG, "null data");
  if (!f) return fail(CSSM_EINVAL_ARG, "null fleet");
  FleetRide ride;
  ride.more = true;
  return fleet_filter_all(f, off, t, y, has_obs, ll_out, ll_t, ess_t, rc_out, ride);
}

// ... and cssm_fleet_summary of the cloud behind every one of those records from the same launch (the IVAL instantiation): a row per
// record, laid out like t -- none for an initial cloud, since none is drawn.
extern "C" int cssm_fleet_filter_intervals_more(cssm_fleet* f, const uint64_t* off, const double* t, const double* y, const uint8_t* has_obs,
                                                double interval, double* ll_out, double* ll_t, int32_t* ess_t, double* state_mean, double* state_lower,
                                                double* state_upper, double* eta_of_mean, double* eta_lower, double* eta_upper, int* rc_out) {
  FLEET_LGCP_REFUSE(f, "cssm_fleet_filter_intervals_more", FLEET_LGCP_SERVED);
  if (!off) return fail(CSSM_EINVAL_ARG, "off is null");
  if (!ll_out || !rc_out) return fail(CSSM_EINVAL_ARG, "ll_out / rc_out is null");
  if (off[0] != 0) return fail(CSSM_EINVAL_ARG, "off[0] must be 0");
  if (!t || !y) return fail(CSSM_EINVAL_ARG, "null data");
  if (!(interval > 0.0 && interval <= 1.0)) return fail(CSSM_EINVAL_ARG, "interval must be in (0, 1]");
  if (!f) return fail(CSSM_EINVAL_ARG, "null fleet");
  const uint32_t S = f->S;
  std::vector<uint8_t> ran(S);   // (a series that fails loses its cloud: asked before the call)
  for (uint32_t k = 0; k < S; ++k) ran[k] = f->live[k];
  FleetRide ride;
  ride.kind = FleetKind::ival; ride.interval = interval; ride.more = true;
  int rc = fleet_filter_all(f, off, t, y, has_obs, ll_out, ll_t, ess_t, rc_out, ride);
  if (rc) return rc;
  const int d = f->d;
  const size_t R = (size_t)off[S], rowsz = (size_t)(d + 1) * 3u;
  const FleetIvOut o{state_mean, state_lower, state_upper, eta_of_mean, eta_lower, eta_upper};
  for (double* p : {state_mean, state_lower, state_upper}) if (p) std::fill(p, p + R * (size_t)d, cssm_nan());
  for (double* p : {eta_of_mean, eta_lower, eta_upper}) if (p) std::fill(p, p + R, cssm_nan());
  const FleetStageView h = fleet_view(ride.st, f->h_stage);   // (the staged launch is still there: its own offsets, the f coefficients of every row)
  fleet_parallel(S, R, [&](size_t lo, size_t hi) {
    for (size_t k = lo; k < hi; ++k) {
      const size_t a = (size_t)off[k], b = (size_t)off[k + 1], r0 = (size_t)h.off[k];
      if (b == a || !ran[k]) continue;
      const FleetSeries& s = f->h_ser[k];
      const size_t nrows = s.err ? (size_t)s.fail_rec : b - a;   // a failure at record s keeps the rows of the records before it
      for (size_t i = 0; i < nrows; ++i) fleet_iv_row(f, (uint32_t)k, ride.out.data() + (r0 + i) * rowsz, fleet_rec_fco(h, d, r0 + i), true, o, a + i);
    }
  });
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
  FLEET_LGCP_REFUSE(f, "cssm_fleet_pmmh_run", FLEET_PMMH_SERVED);
  size_t flat = 0;
  rc = cssm_desc_flatten(desc, nullptr, 0, &flat);
  if (rc) return rc;
  if (flat != n_theta) return fail(CSSM_EINVAL_ARG, "theta0 has %zu entries per chain, the descriptor flattens to %zu", n_theta, flat);
  if (!f) return fail(CSSM_EINVAL_ARG, "null fleet");
  const uint32_t S = f->S;
  const int d = f->d;
  for (uint32_t k = 0; k < S; ++k) {
    if ((rc = fleet_off_step("off", off, k))) return rc;
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
  FleetRide ride;
  int rc = fleet_ensure(f, 0, ride);
  if (rc) return rc;
  const uint32_t S = f->S;
  const FleetStageView h = fleet_view(ride.st, f->h_stage);
  for (uint32_t k = 0; k <= S; ++k) h.off[k] = 0;
  for (uint32_t k = 0; k < S; ++k) h.ctl[k] = CSSM_FLEET_CTL_INIT;
  rc = fleet_launch(f, ride, nullptr, nullptr);
  if (rc) return rc;
  for (uint32_t k = 0; k < S; ++k) { f->live[k] = 1; f->t[k] = t0[k]; f->step[k] = 0u; }
  return CSSM_OK;
}

// FilterInit(mod, resample, initState).initialiseState (model/ParticleFilter.scala:252-271) of the active series, and its posterior form: the
// clouds come from the caller -- one row replicated, or the rows of a posterior sample under the caller's picks or the selection
// cssm_fleet_forecast_posterior makes.  ONE launch without records, as cssm_fleet_init's; a series the call refuses or does not name gets no
// block and stays exactly as it was.
extern "C" int cssm_fleet_init_from(cssm_fleet* f, const uint8_t* active, const double* t0, const uint64_t* moff, const double* x,
                                    const uint32_t* pick, const uint64_t* keys, uint32_t* pick_out, int* rc_out) {
  if (!t0 || !moff || !x || !rc_out) return fail(CSSM_EINVAL_ARG, "null argument (t0, moff, x, rc_out)");
  if (moff[0] != 0) return fail(CSSM_EINVAL_ARG, "moff[0] must be 0");
  if (!f) return fail(CSSM_EINVAL_ARG, "null fleet");
  const uint32_t S = f->S, n = f->n;
  const int d = f->d;
  int rc = CSSM_OK;
  for (uint32_t k = 0; k < S; ++k)
    if ((rc = fleet_off_step("moff", moff, k))) return rc;
  HIP_TRY(hipSetDevice(f->device));
  FleetRide ride;
  ride.from = true; ride.from_M = (size_t)moff[S]; ride.from_picks = pick != nullptr; ride.pick_out = pick_out;
  rc = fleet_ensure(f, 0, ride);
  if (rc) return rc;
  const FleetStageView h = fleet_view(ride.st, f->h_stage);
  std::vector<std::string> msg(S);
  for (uint32_t k = 0; k <= S; ++k) { h.off[k] = 0; h.fr_moff[k] = moff[k]; }
  if (pick) {
    memcpy(h.fr_pick, pick, (size_t)S * n * 4u);
    if (((size_t)S * n) & 1u) h.fr_pick[(size_t)S * n] = 0u;   // (the padding travels too)
  }
  fleet_parallel(S, (size_t)moff[S] + (pick ? (size_t)S * n : 0u), [&](size_t lo, size_t hi) {
    for (size_t k = lo; k < hi; ++k) {
      const size_t ma = (size_t)moff[k], M = (size_t)moff[k + 1] - ma;
      h.ctl[k] = 0u; h.fr_keys[k] = keys ? keys[k] : 0ull; rc_out[k] = CSSM_OK;
      std::fill(h.fr_x + ma * (size_t)d, h.fr_x + (ma + M) * (size_t)d, 0.0);   // (the rows of a series that is not served travel as zeros)
      if (active && !active[k]) continue;                                      // untouched: nothing of it is read
      auto refuse = [&](const std::string& why) { rc_out[k] = CSSM_EINVAL_ARG; msg[k] = why; };
      if (M == 0) { refuse("no state to start from (M = 0)"); continue; }
      if (M > 0xffffffffull) { refuse("more than 2^32 - 1 rows"); continue; }
      if (!std::isfinite(t0[k])) { refuse("t0 is not finite"); continue; }
      const double* xs = x + ma * (size_t)d;
      for (size_t m = 0; m < M && !rc_out[k]; ++m)
        for (int c = 0; c < d; ++c)
          if (!std::isfinite(xs[m * d + c])) { refuse("x row " + std::to_string(m) + ": component " + std::to_string(c) + " is not finite"); break; }
      if (rc_out[k]) continue;
      if (M > 1 && !pick && !keys) { refuse("M = " + std::to_string(M) + " rows and neither pick nor keys to choose among them"); continue; }
      if (pick)
        for (uint32_t i = 0; i < n; ++i)
          if (pick[k * n + i] >= M) {
            refuse("pick[" + std::to_string(i) + "] = " + std::to_string(pick[k * n + i]) + " is not below M = " + std::to_string(M));
            break;
          }
      if (rc_out[k]) continue;
      memcpy(h.fr_x + ma * (size_t)d, xs, M * (size_t)d * 8u);
      h.ctl[k] = CSSM_FLEET_CTL_INIT | CSSM_FLEET_CTL_FROM;
    }
  });
  if (S & 1u) h.ctl[S] = 0u;
  rc = fleet_launch(f, ride, nullptr, nullptr);
  if (rc) return rc;
  for (uint32_t k = 0; k < S; ++k) {
    const bool served = (h.ctl[k] & CSSM_FLEET_CTL_FROM) != 0u;
    if (served) { f->live[k] = 1; f->t[k] = t0[k]; f->step[k] = 0u; }
    else if (pick_out) std::fill(pick_out + (size_t)k * n, pick_out + (size_t)(k + 1) * n, 0u);
  }
  for (uint32_t k = 0; k < S; ++k)   // (the call succeeds; the message names the first refused series)
    if (rc_out[k]) { (void)fail(CSSM_EINVAL_ARG, "series %u: %s", k, msg[k].c_str()); break; }
  return CSSM_OK;
}

// EXTENSION (the reference has no operation that writes one filter's cloud from another's; SMC2's resampling and adoption need it):
// dst series k <- src series map[k], simultaneously.  The moved series are compacted into a table of moves (staged like a launch's
// records) and k_fleet_copy gathers them (cssm_fleet_copy.hip.h).  Two fleets: one launch behind an event on the source's stream, every
// cloud straight into the half its observation index selects.  One fleet: that half is, in lockstep use, the destination's own live
// half, which another block may be reading as ITS source -- and nothing waits on another block inside a kernel.  So the first launch
// writes every moved cloud into the destination's NON-live half (nobody reads one: conflict-free for any map) and the ancestors and
// scalars into d_copy; the second launch settles, within each series, the clouds whose required half is the other one and brings
// ancestors and scalars home.  A destination without a cloud has no live half: its cloud goes straight where it belongs.
extern "C" int cssm_fleet_copy_series(cssm_fleet* dst, cssm_fleet* src, const uint64_t* umap, int flags, int* rc_out) {
  const int64_t* map = reinterpret_cast<const int64_t*>(umap);   // (signed entries in the header's unsigned type: include/cssm_pf.h)
  if (!dst || !src || !umap || !rc_out) return fail(CSSM_EINVAL_ARG, "null argument (dst, src, map, rc_out)");
  if (flags & ~CSSM_FLEET_COPY_KEYS) return fail(CSSM_EINVAL_ARG, "cssm_fleet_copy_series: unknown flag bits 0x%x", (unsigned)(flags & ~CSSM_FLEET_COPY_KEYS));
  const uint32_t S = dst->S, n = dst->n;
  const bool same = src == dst;
  for (uint32_t k = 0; k < S; ++k)
    if (map[k] < CSSM_FLEET_COPY_KEEP || map[k] >= (int64_t)src->S)
      return fail(CSSM_EINVAL_ARG, "map[%u] = %lld is neither CSSM_FLEET_COPY_KEEP nor a series of the source (0 .. %u)", k, (long long)map[k], src->S - 1u);
  if (src->n != n) return fail(CSSM_EINVAL_ARG, "the fleets hold clouds of different sizes (%u and %u particles)", src->n, n);
  if (src->device != dst->device) return fail(CSSM_EINVAL_ARG, "the fleets live on different devices (%d and %d)", src->device, dst->device);
  if (src->lgcp != dst->lgcp) return fail(CSSM_EINVAL_ARG, "one fleet is an LGCP fleet and the other is not");
  {
    const HostModel &a = src->base, &b = dst->base;
    std::string diff;
    auto differs = [&](const char* what) { diff += diff.empty() ? "" : ", "; diff += what; };
    bool comps = a.d == b.d && a.n_leaves == b.n_leaves;
    for (int c = 0; comps && c < a.d; ++c)
      comps = a.comp[c].kind == b.comp[c].kind && a.comp[c].leaf == b.comp[c].leaf && a.comp[c].idx == b.comp[c].idx &&
              a.comp[c].f_kind == b.comp[c].f_kind && a.comp[c].period == b.comp[c].period;
    for (int w = 0; comps && w < CSSM_MAX_DIM / 4; ++w) comps = a.mk.comp[w] == b.mk.comp[w];
    if (!comps) differs("the components (cssm_model_structure)");
    if (a.obs_kind != b.obs_kind) differs("obs_kind");
    if (a.obs_df != b.obs_df) differs("obs_df");
    if (a.precision != b.precision) differs("lgcp_precision");
    if (!diff.empty()) return fail(CSSM_EINVAL_DESC, "the fleets differ in model structure: %s", diff.c_str());
  }
  const int d = dst->d;
  const size_t dn = (size_t)d * n;
  std::vector<uint32_t> moved;
  int64_t first_dead = -1;
  for (uint32_t k = 0; k < S; ++k) {
    rc_out[k] = CSSM_OK;
    const int64_t j = map[k];
    if (j < 0 || (same && j == (int64_t)k)) continue;
    if (!src->live[(size_t)j]) { rc_out[k] = CSSM_ESTATE; if (first_dead < 0) first_dead = (int64_t)k; continue; }
    moved.push_back(k);
  }
  const size_t M = moved.size();
  if (M) {
    HIP_TRY(hipSetDevice(dst->device));
    const size_t table = M * sizeof(FleetCopyMove), anc_bytes = fleet_pad8((size_t)S * n * 4u);
    if (!dst->h_stage.reserve(2u * table, true) || !dst->d_stage.reserve(2u * table, true)) return fail(CSSM_ENOMEM, "fleet copy: %zu bytes of moves", 2u * table);
    if (same && !dst->d_copy.reserve(anc_bytes + (size_t)S * sizeof(FleetSeries), false))
      return fail(CSSM_ENOMEM, "fleet copy: %zu bytes between its two launches", anc_bytes + (size_t)S * sizeof(FleetSeries));
    if (!same && !dst->ev_copy && hipEventCreateWithFlags(&dst->ev_copy, hipEventDisableTiming) != hipSuccess) return fail(CSSM_EHIP, "hipEventCreate");
    FleetCopyMove* h1 = dst->h_stage.at<FleetCopyMove>();
    FleetCopyMove* h2 = h1 + M;
    for (size_t q = 0; q < M; ++q) {
      const uint32_t k = moved[q], j = (uint32_t)map[k];
      const uint32_t need = src->step[j] & 1u;                                              // the half the source's observation index selects
      const uint32_t first = (same && dst->live[k]) ? 1u - (dst->step[k] & 1u) : need;     // one fleet: the destination's non-live half
      h1[q] = FleetCopyMove{((size_t)j * 2u + need) * dn, ((size_t)k * 2u + first) * dn, j, k, CSSM_FLEET_COPY_CLOUD, 0u};
      h2[q] = FleetCopyMove{((size_t)k * 2u + first) * dn, ((size_t)k * 2u + need) * dn, k, k, first != need ? CSSM_FLEET_COPY_CLOUD : 0u, 0u};
    }
    if (!same) {   // behind everything the source's stream still holds
      HIP_TRY(hipEventRecord(dst->ev_copy, src->stream));
      HIP_TRY(hipStreamWaitEvent(dst->stream, dst->ev_copy, 0));
    }
    HIP_TRY(hipEventRecord(dst->ev[EV_CALL_BEGIN], dst->stream));
    HIP_TRY(hipMemcpyAsync(dst->d_stage.p, dst->h_stage.p, (same ? 2u : 1u) * table, hipMemcpyHostToDevice, dst->stream));
    FleetCopyArgs a{};
    a.dn = (uint32_t)dn; a.n = n; a.tiles = (uint32_t)((dn + CSSM_FLEET_COPY_TILE - 1u) / CSSM_FLEET_COPY_TILE);
    a.moves = dst->d_stage.at<FleetCopyMove>();
    a.src_state = src->state.at<double>(); a.dst_state = dst->state.at<double>();
    a.src_anc = src->anc.at<uint32_t>(); a.src_ser = src->ser.at<FleetSeries>();
    a.dst_anc = same ? dst->d_copy.at<uint32_t>() : dst->anc.at<uint32_t>();
    a.dst_ser = same ? dst->d_copy.at<FleetSeries>(anc_bytes) : dst->ser.at<FleetSeries>();
    int hrc = fleet_copy_launch(a, (uint32_t)M, dst->stream);
    if (!hrc && same) {   // settle: every block reads only what the first launch finished, within its own series
      a.moves += M;
      a.src_state = a.dst_state;
      a.src_anc = a.dst_anc; a.src_ser = a.dst_ser;
      a.dst_anc = dst->anc.at<uint32_t>(); a.dst_ser = dst->ser.at<FleetSeries>();
      hrc = fleet_copy_launch(a, (uint32_t)M, dst->stream);
    }
    if (hrc) return fail(CSSM_EHIP, "k_fleet_copy: %s", hipGetErrorString((hipError_t)hrc));
    HIP_TRY(hipEventRecord(dst->ev[EV_CALL_END], dst->stream));
    HIP_TRY(hipStreamSynchronize(dst->stream));
    if (hipEventElapsedTime(&dst->ms_call, dst->ev[EV_CALL_BEGIN], dst->ev[EV_CALL_END]) != hipSuccess) dst->ms_call = -1.f;
    // the host's side of every moved series, read before any is written (the assignment is simultaneous)
    struct Host { HostModel m; double t; uint32_t step; int has_scale; double scale; };
    std::vector<Host> from(M);
    for (size_t q = 0; q < M; ++q) {
      const size_t j = (size_t)map[moved[q]];
      from[q] = Host{src->models[j], src->t[j], src->step[j], src->obs_has_scale[j], src->obs_scale[j]};
    }
    for (size_t q = 0; q < M; ++q) {
      const uint32_t k = moved[q];
      const uint64_t own = dst->models[k].seed;
      dst->models[k] = from[q].m;
      if (!(flags & CSSM_FLEET_COPY_KEYS)) dst->models[k].seed = own;
      dst->t[k] = from[q].t; dst->step[k] = from[q].step; dst->live[k] = 1;
      dst->obs_has_scale[k] = from[q].has_scale; dst->obs_scale[k] = from[q].scale;
      fleet_win_drop(dst, k);
    }
    dst->par_dirty = true;
  } else {
    dst->ms_call = 0.f;
  }
  if (first_dead >= 0)   // (the call succeeds; the message names the first such series)
    (void)fail(CSSM_ESTATE, "series %lld: its source, series %lld, has no cloud (not initialised, or its weights were unusable)", (long long)first_dead,
               (long long)map[first_dead]);
  return CSSM_OK;
}

// stepFilter of the active series, one record each, with the call's rider: ival (cssm_fleet_step_intervals) -- the same launch also
// writes getIntervals of every cloud it moved; fcst (cssm_fleet_step_forecast) -- and forecasts every record before it is stepped; ring
// (cssm_fleet_step_interpolate) -- remembers every cloud it moved in the series' window, and a second launch summarises the last rows of
// the series that ask through the lineages that survive to that cloud
static int fleet_step_all(cssm_fleet* f, const uint8_t* active, const double* t, const double* y, const uint8_t* has_obs,
                          double* ll_out, int32_t* ess_out, int* rc_out, FleetRide& ride) {
  const uint32_t S = f->S;
  const int d = f->d;
  bool any_live = false;
  for (uint32_t k = 0; k < S; ++k) any_live = any_live || f->live[k];
  if (!any_live) return fail(CSSM_ESTATE, "no series of the fleet is initialised (cssm_fleet_init / cssm_fleet_ll_filter first)");
  HIP_TRY(hipSetDevice(f->device));
  auto runs = [&](uint32_t k) { return (!active || active[k]) && f->live[k]; };
  const bool ival = ride.kind == FleetKind::ival, fcst = ride.kind == FleetKind::fcst, ring = ride.kind == FleetKind::ring;
  const uint32_t W = f->win_slices;
  auto lag_of = [&](uint32_t k) { return ride.lag ? ride.lag[k] : ride.max_lag; };
  size_t R = 0;
  for (uint32_t k = 0; k < S; ++k) {
    R += runs(k) ? 1u : 0u;
    if (ring && runs(k) && lag_of(k) != CSSM_FLEET_NO_ROWS) ride.win_Q += 1u;
  }
  if (ring) ride.win_L = std::min<size_t>((size_t)ride.max_lag + 1u, W);   // (a window never returns more rows than it has slots)
  ride.step = true;
  int rc = CSSM_OK;
  std::vector<size_t> toff;   // (LGCP fleet, f depends on time) where series k's rows start in the launch's sub-step table (doubles)
  if (f->lgcp && f->base.lgcp_tdep) {
    toff.assign((size_t)S + 1u, 0);
    for (uint32_t k = 0; k < S; ++k) toff[k + 1] = toff[k] + (runs(k) ? fleet_lgcp_rows(f->models[k], f->t[k], t + k, 1) : 0u);
    if ((rc = fleet_lgcp_table_fits(toff[S]))) return rc;
    ride.fsub_doubles = toff[S];
  }
  rc = fleet_ensure(f, R, ride);
  if (rc) return rc;
  const FleetStageView h = fleet_view(ride.st, f->h_stage);
  h.off[0] = 0;
  for (uint32_t k = 0; k < S; ++k) { h.ctl[k] = 0u; h.off[k + 1] = h.off[k] + (runs(k) ? 1u : 0u); }
  std::atomic<int> pack_rc{CSSM_OK};
  fleet_parallel(S, R, [&](size_t lo, size_t hi) {
    for (size_t k = lo; k < hi; ++k) {
      if (h.off[k + 1] == h.off[k]) continue;
      unsigned char* dst = h.recs + (size_t)h.off[k] * ride.st.rec_bytes;
      if (f->lgcp) {
        std::vector<double> tab;
        const int prc = fleet_pack_rec_lgcp(f->models[k], f->t[k], t[k], f->step[k], dst, tab, toff.empty() ? 0u : toff[k]);
        if (prc) pack_rc = prc;
        if (!tab.empty() && tab.size() == toff[k + 1] - toff[k]) memcpy(h.fsub + toff[k], tab.data(), tab.size() * 8u);
        else if (!tab.empty()) pack_rc = CSSM_ENOMEM;
        continue;
      }
      fleet_pack_rec(f->models[k], f->t[k], t[k], y[k], has_obs ? (int)has_obs[k] : 1, f->step[k], dst);
    }
  });
  if (pack_rc) return fail(pack_rc, "fleet: the sub-step table of the launch could not be built");
  if (fcst) {
    fleet_fc_series(f, ride, h, runs);
    for (uint32_t k = 0; k < S; ++k)
      if (runs(k)) fleet_fc_record(f, ride, h, k, (size_t)h.off[k], k, f->step[k], f->t[k], t[k], y[k], has_obs ? (int)has_obs[k] : 1);
  }
  if (ival) memset(h.fco0, 0, (size_t)S * d * 8u);   // (no launch of a step draws a cloud: the f coefficients of a t0 are not read)
  std::vector<uint32_t> w_req_of;                    // ring: series k's request, or none
  if (ring) {
    // the ring arithmetic, here and nowhere else: a window that is not continuous restarts at slot 0 with the cloud the series holds now
    // as its base slice (F at the series' clock, no ancestors); the record's slot is the one behind the newest, modulo the slices.  What
    // is noted per slot is noted now (a series that fails loses its window anyway); head / depth move once the launch has succeeded.
    w_req_of.assign(S, CSSM_FLEET_NO_ROWS);
    const size_t L = ride.win_L;
    size_t q = 0;
    for (uint32_t k = 0; k < S; ++k) {
      h.w_base[k] = 0u;
      if (!runs(k)) continue;
      const size_t r = (size_t)h.off[k], w0 = (size_t)k * W;
      const bool restart = !f->win_on[k];
      const uint32_t head = restart ? 0u : f->win_head[k], depth = restart ? 0u : f->win_depth[k];
      const uint32_t slot = (head + 1u) % W, depth1 = std::min(depth + 1u, W - 1u);
      if (restart) {
        h.ctl[k] |= CSSM_FLEET_CTL_BASE;
        StepRec r0;
        cssm_build_rec(&f->models[k], f->t[k], f->t[k], 0.0, 0, 0u, &r0);   // F at the base slice's time
        for (int c = 0; c < d; ++c) f->win_fco[w0 * d + c] = r0.fco[c];
        f->win_res[w0] = 0;
      }
      h.w_slot[r] = slot;
      const double* fco = fleet_rec_fco(h, d, r);
      for (int c = 0; c < d; ++c) f->win_fco[(w0 + slot) * d + c] = fco[c];
      f->win_res[w0 + slot] = (has_obs ? has_obs[k] : 1) ? 1 : 0;
      const uint32_t lg = lag_of(k);
      if (lg == CSSM_FLEET_NO_ROWS) continue;
      const uint32_t nrows = std::min(lg, depth1) + 1u;       // <= slices: L holds them
      w_req_of[k] = (uint32_t)q;
      h.w_req[q] = FleetWinReq{k, nrows};
      for (uint32_t j = 0; j < (uint32_t)L; ++j) {
        const uint32_t sj = (slot + W - (j % W)) % W;           // (rows beyond nrows are not walked: their words only travel)
        h.w_words[q * L + j] = j < nrows ? (sj | (f->win_res[w0 + sj] ? CSSM_FLEET_WIN_RESAMPLED : 0u)) : 0u;
        for (int c = 0; c < d; ++c) h.w_fco[(q * L + j) * d + c] = j < nrows ? f->win_fco[(w0 + sj) * d + c] : 0.0;
      }
      ++q;
    }
    if (R & 1u) h.w_slot[R] = 0u;                              // (the padding travels too)
    if (S & 1u) h.w_base[S] = 0u;
    if ((ride.win_Q * L) & 1u) h.w_words[ride.win_Q * L] = 0u;
  }
  rc = fleet_launch(f, ride, nullptr, nullptr);
  if (rc) {
    if (ring) for (uint32_t k = 0; k < S; ++k) if (runs(k)) fleet_win_drop(f, k);
    return rc;
  }
  for (uint32_t k = 0; k < S; ++k) {
    if (ride.fc_rc_out) ride.fc_rc_out[k] = ride.fc_rc[k];
    if (active && !active[k]) { rc_out[k] = CSSM_OK; continue; }            // untouched
    if (!f->live[k]) { rc_out[k] = CSSM_ESTATE; continue; }                 // no cloud: never initialised, or failed since
    const FleetSeries& s = f->h_ser[k];
    if (s.err) { rc_out[k] = CSSM_ENONFINITE; f->live[k] = 0; fleet_win_drop(f, k); continue; }
    rc_out[k] = CSSM_OK; f->t[k] = t[k]; f->step[k] += 1u;
    if (ll_out) ll_out[k] = s.ll;
    if (ess_out) ess_out[k] = s.ess;
    const size_t r = (size_t)h.off[k];
    if (ival) fleet_iv_row(f, k, ride.out.data() + (size_t)k * (d + 1) * 3u, fleet_rec_fco(h, d, r), true, ride.ivo, k);
    if (fcst) fleet_fc_row(d, ride.out.data() + (size_t)k * (d + 2) * 3u, ride.pit.data() + 2 * (size_t)k, (h.flags[r] & CSSM_FLEET_FC_ON) != 0u, ride.fco, k);
    if (ring) {
      const bool restart = !f->win_on[k];
      f->win_head[k] = ((restart ? 0u : f->win_head[k]) + 1u) % W;
      f->win_depth[k] = std::min((restart ? 0u : f->win_depth[k]) + 1u, W - 1u);
      f->win_on[k] = 1;
      const uint32_t q = w_req_of[k];
      const uint32_t nrows = q == CSSM_FLEET_NO_ROWS ? 0u : h.w_req[q].rows;
      if (ride.rows_out) ride.rows_out[k] = nrows;
      if (q == CSSM_FLEET_NO_ROWS) continue;                   // stepped and remembered, not summarised: nothing of its rows is written
      const size_t L = ride.win_L, Lc = (size_t)ride.max_lag + 1u;
      for (size_t j = 0; j < Lc; ++j) {
        const bool ok = j < nrows;
        const size_t at = q * L + (ok ? j : 0u);
        fleet_iv_row(f, k, ride.out.data() + at * (size_t)(d + 1) * 3u, h.w_fco + at * d, ok, ride.ivo, (size_t)k * Lc + j);
      }
    }
  }
  if (!ride.scale_msg.empty()) (void)fail(CSSM_EINVAL_ARG, "%s", ride.scale_msg.c_str());   // (the call succeeds)
  return CSSM_OK;
}

extern "C" int cssm_fleet_step(cssm_fleet* f, const uint8_t* active, const double* t, const double* y, const uint8_t* has_obs,
                               double* ll_out, int32_t* ess_out, int* rc_out) {
  if (!f || !t || (!y && !f->lgcp) || !rc_out) return fail(CSSM_EINVAL_ARG, "null argument");
  FleetRide ride;
  return fleet_step_all(f, active, t, y, has_obs, ll_out, ess_out, rc_out, ride);
}

// filterStream + getIntervals (examples/Filtering.scala:24-31, one observation per sensor per call): cssm_fleet_step, and the summaries of
// every cloud it moved from the same launch.  The entries of a series that is inactive, has no cloud or fails are not written.
extern "C" int cssm_fleet_step_intervals(cssm_fleet* f, const uint8_t* active, const double* t, const double* y, const uint8_t* has_obs, double interval,
                                         double* ll_out, int32_t* ess_out, double* state_mean, double* state_lower, double* state_upper,
                                         double* eta_of_mean, double* eta_lower, double* eta_upper, int* rc_out) {
  FLEET_LGCP_REFUSE(f, "cssm_fleet_step_intervals", FLEET_LGCP_SERVED);
  if (!t || !y || !rc_out) return fail(CSSM_EINVAL_ARG, "null argument");
  if (!(interval > 0.0 && interval <= 1.0)) return fail(CSSM_EINVAL_ARG, "interval must be in (0, 1]");
  if (!f) return fail(CSSM_EINVAL_ARG, "null fleet");
  FleetRide ride;
  ride.kind = FleetKind::ival; ride.interval = interval;
  ride.ivo = FleetIvOut{state_mean, state_lower, state_upper, eta_of_mean, eta_lower, eta_upper};
  return fleet_step_all(f, active, t, y, has_obs, ll_out, ess_out, rc_out, ride);
}

// getMeanForecast over a filterStream, one observation per sensor per call: cssm_fleet_step -- the same arguments, bits and statuses -- and
// before the record is stepped cssm_fleet_forecast of its time, from the same launch.  The entries of a series that is inactive, has no
// cloud or fails are not written.
extern "C" int cssm_fleet_step_forecast(cssm_fleet* f, const uint8_t* active, const double* t, const double* y, const uint8_t* has_obs,
                                        const uint64_t* keys, double interval, double* ll_out, int32_t* ess_out, double* state_mean,
                                        double* state_lower, double* state_upper, double* eta_mean, double* eta_lower, double* eta_upper,
                                        double* obs_mean, double* obs_lower, double* obs_upper, int32_t* obs_below, int32_t* obs_equal,
                                        int* rc_out, int* fc_rc_out) {
  FLEET_LGCP_REFUSE(f, "cssm_fleet_step_forecast", FLEET_LGCP_SERVED);
  if (!t || !y || !rc_out || !fc_rc_out) return fail(CSSM_EINVAL_ARG, "null argument (t, y, rc_out, fc_rc_out)");
  if (!(interval > 0.0 && interval <= 1.0)) return fail(CSSM_EINVAL_ARG, "interval must be in (0, 1]");
  if (!f) return fail(CSSM_EINVAL_ARG, "null fleet");
  FleetRide ride;
  ride.kind = FleetKind::fcst; ride.interval = interval; ride.keys = keys; ride.fc_rc_out = fc_rc_out;
  ride.fco = FleetFcOut{state_mean, state_lower, state_upper, eta_mean, eta_lower, eta_upper, obs_mean, obs_lower, obs_upper, obs_below, obs_equal};
  return fleet_step_all(f, active, t, y, has_obs, ll_out, ess_out, rc_out, ride);
}

// The window cssm_fleet_step_interpolate remembers in: `slices` slots per series, a cloud and its ancestors each -- S x slices x N x
// (8 d + 4) bytes.  Every window restarts.
extern "C" int cssm_fleet_window(cssm_fleet* f, uint32_t slices) {
  FLEET_LGCP_REFUSE(f, "cssm_fleet_window", FLEET_LGCP_SERVED);
  if (slices == 1u) return fail(CSSM_EINVAL_ARG, "a window of 1 slice remembers no record behind its base slice: slices is 0 (no window) or at least 2");
  if (!f) return fail(CSSM_EINVAL_ARG, "null fleet");
  HIP_TRY(hipSetDevice(f->device));
  HIP_TRY(hipStreamSynchronize(f->stream));
  f->win.release();
  f->win_slices = 0;
  f->win_on.clear(); f->win_res.clear(); f->win_head.clear(); f->win_depth.clear(); f->win_fco.clear();
  if (slices == 0u) return CSSM_OK;
  const size_t per = (size_t)f->S * f->n * (8u * (size_t)f->d + 4u);
  if (slices > 0x7fffffffu || (size_t)slices > (~(size_t)0) / per)
    return fail(CSSM_ENOMEM, "fleet window: %u slices of %zu bytes each do not fit any memory", slices, per);
  const size_t bytes = per * slices;
  if (!f->win.reserve(bytes, false)) {
    (void)hipGetLastError();   // (the fleet goes on without a window)
    return fail(CSSM_ENOMEM, "fleet window: %zu bytes of history (S x slices x N x (8 d + 4) = %u x %u x %u x %d) do not fit the device", bytes, f->S,
                slices, f->n, 8 * f->d + 4);
  }
  const size_t slots = (size_t)f->S * slices;
  f->win_on.assign(f->S, 0); f->win_head.assign(f->S, 0u); f->win_depth.assign(f->S, 0u);
  f->win_res.assign(slots, 0); f->win_fco.assign(slots * (size_t)f->d, 0.0);
  f->win_slices = slices;
  return CSSM_OK;
}

extern "C" uint32_t cssm_fleet_window_depth(const cssm_fleet* f, uint32_t k) { return (f && k < f->S && f->win_slices) ? f->win_depth[k] : 0u; }

// FilterInterpolate as the stream it is (ParticleFilter.interpolate, model/ParticleFilter.scala:281-310; one stepInterpolate per
// observation): cssm_fleet_step -- the same arguments, bits and statuses -- which also remembers every cloud it moved and its ancestors in
// the series' window, and a second launch that summarises, for the series that ask, the last lag + 1 time indices through the lineages
// that survive to the cloud just written.  What needs no fleet is refused first, so that it is refused on any host.
extern "C" int cssm_fleet_step_interpolate(cssm_fleet* f, const uint8_t* active, const double* t, const double* y, const uint8_t* has_obs,
                                           const uint32_t* lag, uint32_t max_lag, double interval, double* ll_out, int32_t* ess_out,
                                           uint32_t* rows_out, double* state_mean, double* state_lower, double* state_upper, double* eta_of_mean,
                                           double* eta_lower, double* eta_upper, int* rc_out) {
  FLEET_LGCP_REFUSE(f, "cssm_fleet_step_interpolate", FLEET_LGCP_SERVED);
  if (!t || !y || !rc_out) return fail(CSSM_EINVAL_ARG, "null argument (t, y, rc_out)");
  if (!(interval > 0.0 && interval <= 1.0)) return fail(CSSM_EINVAL_ARG, "interval must be in (0, 1]");
  if (max_lag == CSSM_FLEET_NO_ROWS) return fail(CSSM_EINVAL_ARG, "max_lag = %u is CSSM_FLEET_NO_ROWS, not a lag", max_lag);
  for (uint32_t k = 0; lag && k < (f ? f->S : 1u); ++k)   // (a fleet has one series at least: lag[0] can be looked at without one)
    if (lag[k] > max_lag && lag[k] != CSSM_FLEET_NO_ROWS)
      return fail(CSSM_EINVAL_ARG, "lag[%u] = %u is above max_lag = %u (CSSM_FLEET_NO_ROWS asks for no rows)", k, lag[k], max_lag);
  if (!f) return fail(CSSM_EINVAL_ARG, "null fleet");
  if (!f->win_slices) return fail(CSSM_ESTATE, "the fleet has no window to remember in (cssm_fleet_window first)");
  FleetRide ride;
  ride.kind = FleetKind::ring; ride.interval = interval; ride.lag = lag; ride.max_lag = max_lag; ride.rows_out = rows_out;
  ride.ivo = FleetIvOut{state_mean, state_lower, state_upper, eta_of_mean, eta_lower, eta_upper};
  return fleet_step_all(f, active, t, y, has_obs, ll_out, ess_out, rc_out, ride);
}

extern "C" int cssm_fleet_step_interpolate_last_ms(cssm_fleet* f, double* ms2) {
  if (!f || !ms2) return fail(CSSM_EINVAL_ARG, "null argument");
  if (!f->win_ran) return fail(CSSM_ESTATE, "no streaming interpolation has run on this fleet (cssm_fleet_step_interpolate first)");
  ms2[0] = f->ms_win[0]; ms2[1] = f->ms_win[1];
  return CSSM_OK;
}

// cssm_fleet_summary as staged in d_sm: [S][d] f coefficients | [S][d + 1][3] results | [S] buffer numbers (u32, padded to 8 bytes)
struct FleetSmStage {
  size_t out, out_bytes, cur, bytes;
};

extern "C" int cssm_fleet_summary(cssm_fleet* f, double interval, double* state_mean, double* state_lower, double* state_upper,
                                  double* eta_of_mean, double* eta_lower, double* eta_upper) {
  if (!f) return fail(CSSM_EINVAL_ARG, "null fleet");
  if (!(interval > 0.0 && interval <= 1.0)) return fail(CSSM_EINVAL_ARG, "interval must be in (0, 1]");
  HIP_TRY(hipSetDevice(f->device));
  const uint32_t S = f->S, n = f->n;
  const int d = f->d, rows = d + 1;
  FleetSmStage st;
  st.out = (size_t)S * d * 8u; st.out_bytes = (size_t)S * rows * 24u; st.cur = st.out + st.out_bytes; st.bytes = st.cur + fleet_pad8((size_t)S * 4u);
  if (!f->d_sm.reserve(st.bytes, false)) return fail(CSSM_ENOMEM, "fleet summary buffers");
  std::vector<double> hbuf(st.bytes / 8u, 0.0);
  double* h_fco = hbuf.data();
  const double* h_out = fleet_at<double>(hbuf.data(), st.out);
  uint32_t* h_cur = fleet_at<uint32_t>(hbuf.data(), st.cur);
  fleet_parallel(S, (size_t)S * 4, [&](size_t lo, size_t hi) {
    for (size_t k = lo; k < hi; ++k) {
      StepRec r;
      cssm_build_rec(&f->models[k], f->t[k], f->t[k], 0.0, 0, f->step[k], &r);   // F(t) of the series' own time
      for (int c = 0; c < d; ++c) h_fco[k * d + c] = r.fco[c];
      h_cur[k] = f->live[k] ? (f->step[k] & 1u) : 0xffffffffu;
    }
  });
  const FleetRanks r = fleet_ranks(n, interval);
  HIP_TRY(hipEventRecord(f->ev[EV_SUMMARY_BEGIN], f->stream));
  HIP_TRY(hipMemcpyAsync(f->d_sm.p, hbuf.data(), st.bytes, hipMemcpyHostToDevice, f->stream));
  DISPATCH_D(d, hipLaunchKernelGGL(k_fleet_summary<D>, dim3(S, rows), dim3(CSSM_BLOCK), (size_t)r.np2 * 8u, f->stream, f->state.at<double>(),
                                   f->anc.at<uint32_t>(), f->d_sm.at<const uint32_t>(st.cur), f->d_sm.at<const double>(), n, r.np2, f->base.mk,
                                   r.rk.lo_state, r.rk.hi_state, r.rk.lo_eta, r.rk.hi_eta, f->d_sm.at<double>(st.out)));
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(fleet_at<double>(hbuf.data(), st.out), f->d_sm.at<double>(st.out), st.out_bytes, hipMemcpyDeviceToHost, f->stream));
  HIP_TRY(hipEventRecord(f->ev[EV_SUMMARY_END], f->stream));
  HIP_TRY(hipStreamSynchronize(f->stream));
  if (hipEventElapsedTime(&f->ms_summary, f->ev[EV_SUMMARY_BEGIN], f->ev[EV_SUMMARY_END]) != hipSuccess) f->ms_summary = -1.f;
  const FleetIvOut o{state_mean, state_lower, state_upper, eta_of_mean, eta_lower, eta_upper};
  for (uint32_t k = 0; k < S; ++k)   // (a series without a cloud: its block wrote NaN)
    fleet_iv_row(f, k, h_out + (size_t)k * rows * 3u, h_fco + (size_t)k * d, f->live[k] != 0, o, k);
  return CSSM_OK;
}

// SimulateData.forecast + summariseForecast (model/Data.scala:196-231) of every series from its current cloud: one upload (offsets,
// keys, observation parameters, buffer numbers, records), one launch whose blocks are the series (k_fleet_forecast), one read-back.
// A call that returns samples runs the fleet in chunks of series whose samples fit fc_samp_max -- never chunks of horizons: a series
// is one block's work.  What a series' own arguments spoil is the series' own: its status, NaN in its outputs, no block for it.
//
// Either forecast as staged in h_fc / d_fc (byte offsets; off is at 0):
//   cssm_fleet_forecast:            [off | keys | observation parameters | buffer numbers | records | results]
//   cssm_fleet_forecast_posterior:  [off | keys | moff | buffer numbers | records | x | rows | picks | results]
// off, moff: S + 1 u64; keys: S u64; buffer numbers: S u32, padded to 8 bytes; records: R compact ones; x: M x d states; rows: M x
// (3 d + 1) constraint-transformed parameters; picks: S x N u32, padded; results: R x [d + 2][3].
struct FleetFcStage {
  size_t keys, op, moff, cur, recs, x, rows, pick, out, out_bytes, bytes;
};
static FleetFcStage fleet_fc_stage(const cssm_fleet* f, size_t R, bool posterior = false, size_t M = 0) {
  const size_t S = f->S, d = (size_t)f->d;
  FleetFcStage st;
  st.keys = (S + 1u) * 8u;
  st.op = st.moff = st.keys + S * 8u;
  st.cur = posterior ? st.moff + (S + 1u) * 8u : st.op + S * sizeof(cssm_obs_params);
  st.recs = st.cur + fleet_pad8(S * 4u);
  st.x = st.recs + R * CSSM_FLEET_REC_BYTES(f->d);
  st.rows = st.x + M * d * 8u;
  st.pick = st.rows + M * (3u * d + 1u) * 8u;
  st.out = st.pick + (posterior ? fleet_pad8(S * f->n * 4u) : 0u);
  st.out_bytes = R * (d + 2u) * 24u;
  st.bytes = st.out + st.out_bytes;
  return st;
}

// the grow-only buffers of both forecasts: `need` bytes of d_fc and of its pinned mirror, the kernels' scratch
static int fleet_fc_ensure(cssm_fleet* f, size_t need) {
  if (!f->h_fc.reserve(need, true)) return fail(CSSM_ENOMEM, "fleet forecast: %zu bytes of pinned staging", need);
  if (!f->d_fc.reserve(need, true)) return fail(CSSM_ENOMEM, "fleet forecast: %zu bytes of records and results", need);
  return fleet_fc_scratch(f);
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
  if (!f->d_fc_samp.reserve(most * samp_row, false)) return fail(CSSM_ENOMEM, "fleet forecast: %zu bytes of samples", most * samp_row);
  return CSSM_OK;
}

// what every launch of either forecast kernel shares: sizes, ranks, the way to a row's order statistics, the fleet's buffers, the
// staged call on the device
static void fleet_fc_args(const cssm_fleet* f, double interval, const FleetFcStage& st, FleetFcLaunch& l) {
  const uint32_t n = f->n;
  const FleetRanks r = fleet_ranks(n, interval);
  l.args.n = n; l.args.np2 = r.np2;
  l.args.select = f->fc_select ? (uint32_t)(f->fc_select == 2) : (uint32_t)(n >= CSSM_FLEET_SELECT_MIN_N);
  l.args.state = f->state.at<double>(); l.args.anc = f->anc.at<uint32_t>();
  l.args.stage = f->d_fc_scratch.at<double>();
  l.args.logtab = f->logtab.at<double>(); l.args.mk = f->base.mk;
  l.args.lo_state = r.rk.lo_state; l.args.hi_state = r.rk.hi_state;
  l.args.lo_eta = r.rk.lo_eta; l.args.hi_eta = r.rk.hi_eta;
  l.args.off = f->d_fc.at<const unsigned long long>();
  l.args.keys = f->d_fc.at<const unsigned long long>(st.keys);
  l.args.cur = f->d_fc.at<const uint32_t>(st.cur);
  l.args.recs = f->d_fc.at<const unsigned char>(st.recs);
  l.args.out = f->d_fc.at<double>(st.out);
  l.d = f->d; l.threads = f->threads; l.stream = f->stream;
}

// the results [R][d + 2][3] into the caller's arrays; a series whose status is not zero reads NaN
static void fleet_fc_scatter(const cssm_fleet* f, const uint64_t* off, const double* h_out, const int* rc_out, const FleetFcOut& o, double* samples) {
  const size_t rowsz = (size_t)(f->d + 2) * 3u, samp = (size_t)(f->d + 3) * f->n;
  for (uint32_t k = 0; k < f->S; ++k) {
    const bool ok = rc_out[k] == CSSM_OK;
    for (size_t r = (size_t)off[k]; r < (size_t)off[k + 1]; ++r) {
      fleet_fc_row(f->d, h_out + r * rowsz, nullptr, ok, o, r);
      if (samples && !ok) std::fill(samples + r * samp, samples + (r + 1) * samp, cssm_nan());
    }
  }
}

// upload `up` bytes of the staged call, run it in the chunks of series `cut` (launch(l) starts one chunk's kernel), bring the samples of
// every chunk and the bytes [back, back + back_bytes) of d_fc home; the device time lands in ms_forecast
template <class Launch>
static int fleet_fc_run(cssm_fleet* f, const uint64_t* off, const std::vector<uint32_t>& cut, FleetFcLaunch& l, size_t up, size_t back, size_t back_bytes,
                        double* samples, const char* kernel, Launch&& launch) {
  const size_t samp_row = (size_t)(f->d + 3) * f->n * 8u;
  HIP_TRY(hipEventRecord(f->ev[EV_FORECAST_BEGIN], f->stream));
  HIP_TRY(hipMemcpyAsync(f->d_fc.p, f->h_fc.p, up, hipMemcpyHostToDevice, f->stream));
  for (size_t c = 0; c + 1 < cut.size(); ++c) {
    const size_t ra = (size_t)off[cut[c]], rb = (size_t)off[cut[c + 1]];
    if (rb == ra) continue;
    l.args.k0 = cut[c]; l.n_series = cut[c + 1] - cut[c];
    l.args.samples = samples ? f->d_fc_samp.at<double>() : nullptr; l.args.samp_r0 = ra;
    const int hrc = launch(l);
    if (hrc) return fail(CSSM_EHIP, "%s: %s", kernel, hipGetErrorString((hipError_t)hrc));
    if (samples) HIP_TRY(hipMemcpyAsync(samples + ra * (size_t)(f->d + 3) * f->n, f->d_fc_samp.p, (rb - ra) * samp_row, hipMemcpyDeviceToHost, f->stream));
    if (samples && c + 2 < cut.size()) HIP_TRY(hipStreamSynchronize(f->stream));   // (the next chunk writes the same buffer)
  }
  HIP_TRY(hipMemcpyAsync(f->h_fc.at<unsigned char>(back), f->d_fc.at<unsigned char>(back), back_bytes, hipMemcpyDeviceToHost, f->stream));
  HIP_TRY(hipEventRecord(f->ev[EV_FORECAST_END], f->stream));
  HIP_TRY(hipStreamSynchronize(f->stream));
  if (hipEventElapsedTime(&f->ms_forecast, f->ev[EV_FORECAST_BEGIN], f->ev[EV_FORECAST_END]) != hipSuccess) f->ms_forecast = -1.f;
  return CSSM_OK;
}

extern "C" int cssm_fleet_forecast(cssm_fleet* f, const uint64_t* off, const double* t, const uint64_t* keys, double interval,
                                   double* state_mean, double* state_lower, double* state_upper, double* eta_mean, double* eta_lower,
                                   double* eta_upper, double* obs_mean, double* obs_lower, double* obs_upper, double* samples, int* rc_out) {
  FLEET_LGCP_REFUSE(f, "cssm_fleet_forecast", FLEET_LGCP_SERVED);
  if (!f || !off || !t || !keys || !rc_out) return fail(CSSM_EINVAL_ARG, "null argument");
  const uint32_t S = f->S;
  int rc = fleet_off_check(off, S);
  if (rc) return rc;
  if (!(interval > 0.0 && interval <= 1.0)) return fail(CSSM_EINVAL_ARG, "interval must be in (0, 1]");
  const size_t R = (size_t)off[S];
  for (uint32_t k = 0; k < S; ++k)
    if (off[k + 1] - off[k] > 0xffffffffull) return fail(CSSM_EINVAL_ARG, "series %u: too many horizons", k);
  if (R == 0) { for (uint32_t k = 0; k < S; ++k) rc_out[k] = CSSM_OK; return CSSM_OK; }
  bool any_live = false;
  for (uint32_t k = 0; k < S; ++k) any_live = any_live || f->live[k];
  if (!any_live) return fail(CSSM_ESTATE, "no series of the fleet is initialised (cssm_fleet_init / cssm_fleet_ll_filter first)");
  HIP_TRY(hipSetDevice(f->device));
  const size_t RB = CSSM_FLEET_REC_BYTES(f->d);
  const FleetFcStage st = fleet_fc_stage(f, R);
  rc = fleet_fc_ensure(f, st.bytes);
  if (rc) return rc;
  unsigned long long* h_off = f->h_fc.at<unsigned long long>();
  unsigned long long* h_keys = f->h_fc.at<unsigned long long>(st.keys);
  cssm_obs_params* h_op = f->h_fc.at<cssm_obs_params>(st.op);
  uint32_t* h_cur = f->h_fc.at<uint32_t>(st.cur);
  unsigned char* h_recs = f->h_fc.at<unsigned char>(st.recs);
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
    rc = fleet_fc_cuts(f, off, samples != nullptr, cut);
    if (rc) return rc;
    FleetFcLaunch l;
    fleet_fc_args(f, interval, st, l);
    l.args.op = f->d_fc.at<const cssm_obs_params>(st.op);
    rc = fleet_fc_run(f, off, cut, l, st.out, st.out, st.out_bytes, samples, "k_fleet_forecast", [](const FleetFcLaunch& q) { return cssm_fleet_forecast_launch(q); });
    if (rc) return rc;
  }
  const FleetFcOut o{state_mean, state_lower, state_upper, eta_mean, eta_lower, eta_upper, obs_mean, obs_lower, obs_upper, nullptr, nullptr};
  fleet_fc_scatter(f, off, f->h_fc.at<const double>(st.out), rc_out, o, samples);
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
  FLEET_LGCP_REFUSE(f, "cssm_fleet_forecast_posterior", FLEET_LGCP_SERVED);
  if (!f || !desc || !moff || !theta || !x || !t0 || !off || !t || !keys || !rc_out) return fail(CSSM_EINVAL_ARG, "null argument");
  const uint32_t S = f->S, n = f->n;
  if (moff[0] != 0) return fail(CSSM_EINVAL_ARG, "moff[0] must be 0");
  if (off[0] != 0) return fail(CSSM_EINVAL_ARG, "off[0] must be 0");
  int rc = CSSM_OK;
  for (uint32_t k = 0; k < S; ++k) {
    if ((rc = fleet_off_step("moff", moff, k))) return rc;
    if ((rc = fleet_off_step("off", off, k))) return rc;
  }
  if (!(interval > 0.0 && interval <= 1.0)) return fail(CSSM_EINVAL_ARG, "interval must be in (0, 1]");
  if (!desc->leaves || desc->n_leaves < 1) return fail(CSSM_EINVAL_DESC, "null model descriptor");
  // the structure (an LGCP descriptor is never a fleet's) and the length of a row: no rows looked at
  rc = cssm_posterior_rows_into(&f->base, desc, theta, n_theta, 0, nullptr);
  if (rc) return rc;
  const size_t R = (size_t)off[S], Mtot = (size_t)moff[S];
  const int d = f->d;
  const size_t RS = 3 * (size_t)d + 1, RB = CSSM_FLEET_REC_BYTES(d);
  HIP_TRY(hipSetDevice(f->device));
  const FleetFcStage st = fleet_fc_stage(f, R, true, Mtot);   // (the caller's picks are uploaded, the drawn ones only read back)
  rc = fleet_fc_ensure(f, st.bytes);
  if (rc) return rc;
  unsigned long long* h_off = f->h_fc.at<unsigned long long>();
  unsigned long long* h_keys = f->h_fc.at<unsigned long long>(st.keys);
  unsigned long long* h_moff = f->h_fc.at<unsigned long long>(st.moff);
  uint32_t* h_cur = f->h_fc.at<uint32_t>(st.cur);
  unsigned char* h_recs = f->h_fc.at<unsigned char>(st.recs);
  double* h_x = f->h_fc.at<double>(st.x);                  // (a series' states are copied here once they are known finite)
  double* h_rows = f->h_fc.at<double>(st.rows);
  uint32_t* h_pick = f->h_fc.at<uint32_t>(st.pick);
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
    fleet_fc_args(f, interval, st, l);
    l.args.op = nullptr;
    FleetFcPost q;
    q.moff = f->d_fc.at<const unsigned long long>(st.moff);
    q.x = f->d_fc.at<const double>(st.x);
    q.rows = f->d_fc.at<const double>(st.rows);
    q.picks = f->d_fc.at<uint32_t>(st.pick);
    q.draw = pick ? 0u : 1u;
    q.obs_df = f->base.obs_df;
    const size_t back = pick_out && !pick ? st.pick : st.out;
    rc = fleet_fc_run(f, off, cut, l, pick ? st.out : st.pick, back, st.bytes - back, samples, "k_fleet_forecast_post",
                      [&](const FleetFcLaunch& ll) { return cssm_fleet_forecast_post_launch(ll, q); });
    if (rc) return rc;
  }
  const FleetFcOut o{state_mean, state_lower, state_upper, eta_mean, eta_lower, eta_upper, obs_mean, obs_lower, obs_upper, nullptr, nullptr};
  fleet_fc_scatter(f, off, f->h_fc.at<const double>(st.out), rc_out, o, samples);
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

// One chunk of cssm_fleet_interpolate -- the series k0 .. k1 - 1, Rc records, Rc + Sc output rows -- as staged in h_ip / d_ip (byte
// offsets; the chunk's own offsets are at 0): [off | records | the f coefficients of every output row | series scalars | results].  The
// first three are uploaded, the last two read back.
struct FleetIpStage {
  size_t recs, fco, ser, out, bytes;
};
static FleetIpStage fleet_ip_stage(const cssm_fleet* f, const uint64_t* off, uint32_t k0, uint32_t k1) {
  const size_t d = (size_t)f->d, Sc = k1 - k0, Rc = (size_t)(off[k1] - off[k0]), Qc = Rc + Sc;
  FleetIpStage st;
  st.recs = (Sc + 1u) * 8u;
  st.fco = st.recs + Rc * CSSM_FLEET_REC_BYTES(f->d);
  st.ser = st.fco + Qc * d * 8u;
  st.out = st.ser + Sc * sizeof(FleetSeries);
  st.bytes = st.out + Qc * (d + 1u) * 24u;
  return st;
}

// FilterInterpolate (model/ParticleFilter.scala:273-311, examples/Interpolate.scala:31-44) of every series: cssm_pf_interpolate per
// series in TWO launches per chunk of series -- the forward pass keeps every cloud and every weighted record's ancestors of a series
// in a slab of its own (k_fleet_series<D, false, true>), the backward pass composes the surviving lineages and summarises every time
// index (k_fleet_lineage, cssm_fleet_interp.hip).  The fleet lends its device, stream, contract table, N, structure, parameters and
// keys; nothing it keeps per series changes.  Chunks: as many series as fit ip_hist_max bytes of history, one at least -- never a
// part of a series.  Per chunk one upload (offsets, records, the f coefficients of every output row), the two launches, one read-back.
// What cssm_fleet_interpolate and cssm_fleet_smooth refuse alike before the fleet is looked at, in that order
static int fleet_ip_check(const uint64_t* off, const double* t, const double* y, const double* ll_out, const int* rc_out, double interval) {
  if (!off) return fail(CSSM_EINVAL_ARG, "off is null");
  if (!ll_out || !rc_out) return fail(CSSM_EINVAL_ARG, "ll_out / rc_out is null");
  if (off[0] != 0) return fail(CSSM_EINVAL_ARG, "off[0] must be 0");
  if (!t || !y) return fail(CSSM_EINVAL_ARG, "null data");
  if (!(interval > 0.0 && interval <= 1.0)) return fail(CSSM_EINVAL_ARG, "interval must be in (0, 1]");
  return CSSM_OK;
}

// n_traj == 0: the interpolation (forward pass, k_fleet_lineage).  n_traj >= 1: cssm_fleet_smooth -- the same chunks, staging and forward
// pass, then k_fleet_backsim and k_fleet_smooth_rows over n_traj trajectories (cssm_fleet_smooth.hip); traj_out may be null.
static int fleet_ip_run(cssm_fleet* f, const uint64_t* off, const double* t, const double* y, const uint8_t* has_obs, double interval, bool pairing,
                        uint32_t n_traj, double* ll_out, const FleetIvOut& o, uint32_t* traj_out, int* rc_out);

extern "C" int cssm_fleet_interpolate(cssm_fleet* f, const uint64_t* off, const double* t, const double* y, const uint8_t* has_obs, double interval,
                                      int flags, double* ll_out, double* state_mean, double* state_lower, double* state_upper, double* eta_of_mean,
                                      double* eta_lower, double* eta_upper, int* rc_out) {
  FLEET_LGCP_REFUSE(f, "cssm_fleet_interpolate", FLEET_LGCP_SERVED);
  if (const int rc = fleet_ip_check(off, t, y, ll_out, rc_out, interval)) return rc;
  if (flags & ~CSSM_INTERP_REFERENCE_PAIRING) return fail(CSSM_EINVAL_ARG, "unknown flag bits 0x%x (CSSM_INTERP_REFERENCE_PAIRING is the only flag)",
                                                          (unsigned)(flags & ~CSSM_INTERP_REFERENCE_PAIRING));
  if (!f) return fail(CSSM_EINVAL_ARG, "null fleet");
  const FleetIvOut o{state_mean, state_lower, state_upper, eta_of_mean, eta_lower, eta_upper};
  return fleet_ip_run(f, off, t, y, has_obs, interval, (flags & CSSM_INTERP_REFERENCE_PAIRING) != 0, 0u, ll_out, o, nullptr, rc_out);
}

// EXTENSION (the reference has no smoother beyond FilterInterpolate): forward filtering, backward simulation of every series --
// cssm_fleet_interpolate's forward pass, then n_traj trajectories drawn backwards through the kept clouds under the contract's backward
// kernel (include/cssm_numerics.h, "backward simulation") and summarised per time index.
extern "C" int cssm_fleet_smooth(cssm_fleet* f, const uint64_t* off, const double* t, const double* y, const uint8_t* has_obs, uint32_t n_traj,
                                 double interval, int flags, double* ll_out, double* state_mean, double* state_lower, double* state_upper,
                                 double* eta_of_mean, double* eta_lower, double* eta_upper, uint32_t* traj_out, int* rc_out) {
  FLEET_LGCP_REFUSE(f, "cssm_fleet_smooth", FLEET_LGCP_SERVED " (the transition over an event is a chain of sub-steps, not one Gaussian)");
  if (const int rc = fleet_ip_check(off, t, y, ll_out, rc_out, interval)) return rc;
  if (flags & CSSM_INTERP_REFERENCE_PAIRING)
    return fail(CSSM_EINVAL_ARG, "cssm_fleet_smooth: CSSM_INTERP_REFERENCE_PAIRING is not offered (row s is time index s; cssm_fleet_interpolate pairs)");
  if (flags) return fail(CSSM_EINVAL_ARG, "cssm_fleet_smooth: unknown flag bits 0x%x (flags must be 0)", (unsigned)flags);
  if (n_traj == 0u || n_traj > CSSM_FLEET_MAX_N)
    return fail(CSSM_EINVAL_ARG, "cssm_fleet_smooth: n_traj must be in [1, CSSM_FLEET_MAX_N = %u] (got %u)", (unsigned)CSSM_FLEET_MAX_N, n_traj);
  if (!f) return fail(CSSM_EINVAL_ARG, "null fleet");
  const FleetIvOut o{state_mean, state_lower, state_upper, eta_of_mean, eta_lower, eta_upper};
  return fleet_ip_run(f, off, t, y, has_obs, interval, false, n_traj, ll_out, o, traj_out, rc_out);
}

extern "C" int cssm_fleet_smooth_last_ms(cssm_fleet* f, double* ms3) {
  if (!f || !ms3) return fail(CSSM_EINVAL_ARG, "null argument");
  if (!f->bs_ran) return fail(CSSM_ESTATE, "no smoothing has run on this fleet (cssm_fleet_smooth first)");
  ms3[0] = f->ms_bs[0]; ms3[1] = f->ms_bs[1]; ms3[2] = f->ms_bs[2];
  return CSSM_OK;
}

// The records of cssm_fleet_if2 and cssm_fleet_pmmh_chains: per (series, record) what does not depend on the parameters (FleetIf2Rec and
// the d f coefficients behind it) -- dt and F(t) as every fleet record has them.
static void fleet_if2_recs(const cssm_fleet* f, const HostModel& probe, const uint64_t* off, const double* t, const double* y, const uint8_t* has_obs,
                           unsigned char* recs) {
  const uint32_t S = f->S;
  const int d = f->d;
  const size_t R = (size_t)off[S], RB = CSSM_FLEET_IF2_REC_BYTES(d);
  const bool own_level = probe.obs_kind == CSSM_OBS_GAUSSIAN || probe.obs_kind == CSSM_OBS_STUDENT_T;
  fleet_parallel(S, R, [&](size_t lo, size_t hi) {
    for (size_t k = lo; k < hi; ++k) {
      const size_t a = (size_t)off[k], b = (size_t)off[k + 1];
      if (b == a) continue;
      double tp = t[a];
      for (size_t s = a + 1; s < b; ++s) tp = (t[s] < tp) ? t[s] : tp;     // data.minBy(_.t).t
      for (size_t s = a; s < b; ++s) {
        StepRec rec;
        cssm_build_rec(&f->base, tp, t[s], y[s], has_obs ? (int)has_obs[s] : 1, (uint32_t)(s - a), &rec);
        FleetIf2Rec h;
        h.y = y[s]; h.ypart = cssm_obs_ypart(probe.obs_kind, y[s], (double)probe.obs_df);
        h.ref = own_level ? 0.0 : cssm_if2_level(probe.obs_kind, y[s], 1.0, (double)probe.obs_df);
        h.dt = rec.dt; h.has_obs = rec.has_obs; h.step = rec.step;
        unsigned char* dst = recs + s * RB;
        memcpy(dst, &h, sizeof h);
        memcpy(dst + sizeof h, rec.fco, (size_t)d * 8u);
        tp = t[s];
      }
    }
  });
}

// EXTENSION (the reference has no likelihood maximiser): iterated filtering (IF2; Ionides, Nguyen, Atchade, Stoev and King 2015) -- S
// independent searches, one workgroup each, every iteration and record of a search inside k_fleet_if2 (cssm_fleet_if2.hip).  The
// arithmetic is the contract's (include/cssm_numerics.h, "iterated filtering").  The fleet lends its device, stream, contract table, N
// and structure; the swarm, the states and the records live in buffers of the call.
#define FLEET_IF2_SERVED "cssm_pmmh_run / cssm_pmmh_run_batched explore the parameters of a single handle's model"
extern "C" int cssm_fleet_if2(cssm_fleet* f, const cssm_model_desc* desc, const double* theta0, const double* swarm0, size_t n_theta,
                              const double* rw_sd, double cooling_fraction_50, uint32_t first_iter, uint32_t n_iters, uint32_t iters_per_launch,
                              const uint64_t* seeds, const uint64_t* off, const double* t, const double* y, const uint8_t* has_obs,
                              double* theta_mean, double* ll, double* swarm_out, double* ll_t, int32_t* ess_t, double* x_out,
                              uint32_t* anc_out, int* rc_out) {
  if (!desc || !rw_sd || !seeds || !off) return fail(CSSM_EINVAL_ARG, "cssm_fleet_if2: null argument (desc, rw_sd, seeds, off)");
  if (!theta0 && !swarm0) return fail(CSSM_EINVAL_ARG, "cssm_fleet_if2: theta0 and swarm0 are both null (a starting row per series, or a whole swarm)");
  if (!theta_mean || !ll || !rc_out) return fail(CSSM_EINVAL_ARG, "cssm_fleet_if2: null output (theta_mean, ll, rc_out)");
  if (off[0] != 0) return fail(CSSM_EINVAL_ARG, "off[0] must be 0");
  if (!t || !y) return fail(CSSM_EINVAL_ARG, "null data");
  for (size_t j = 0; j < n_theta; ++j)
    if (!(rw_sd[j] >= 0.0) || !std::isfinite(rw_sd[j]))
      return fail(CSSM_EINVAL_ARG, "cssm_fleet_if2: rw_sd[%zu] = %g must be finite and not negative (0 keeps the slot fixed)", j, rw_sd[j]);
  if (n_iters < 1u || n_iters > 1000000u) return fail(CSSM_EINVAL_ARG, "cssm_fleet_if2: n_iters must be in [1, 1000000] (got %u)", n_iters);
  if ((uint64_t)first_iter + n_iters > (1ull << 31)) return fail(CSSM_EINVAL_ARG, "cssm_fleet_if2: first_iter + n_iters must not exceed 2^31");
  std::vector<double> cool(n_iters);                            // one array for the kernel and for whoever restates the search
  if (const int crc = cssm_fleet_if2_cooling(cooling_fraction_50, first_iter, n_iters, cool.data())) return crc;
  HostModel probe;
  int rc = cssm_build_model(&probe, desc, false);
  if (rc) return rc;
  if (probe.obs_kind == CSSM_OBS_LGCP)
    return fail(CSSM_EINVAL_DESC, "cssm_fleet_if2: the LGCP observation model (sub-stepped events) is not served; " FLEET_IF2_SERVED);
  If2Map map;
  if ((rc = cssm_if2_map_build(desc, &map))) return rc;
  if ((size_t)map.n_theta != n_theta)
    return fail(CSSM_EINVAL_ARG, "cssm_fleet_if2: n_theta = %zu, the descriptor flattens to %d (cssm_desc_flatten)", n_theta, (int)map.n_theta);
  FLEET_LGCP_REFUSE(f, "cssm_fleet_if2", FLEET_IF2_SERVED);
  if (!f) return fail(CSSM_EINVAL_ARG, "null fleet");
  const uint32_t S = f->S, n = f->n;
  const int d = f->d;
  for (uint32_t k = 0; k < S; ++k) {
    if ((rc = fleet_off_step("off", off, k))) return rc;
    if (off[k + 1] - off[k] > 0xfffffffeull) return fail(CSSM_EINVAL_ARG, "series %u: too many records", k);
  }
  {   // the structure must be the fleet's
    HostModel same = f->base;
    rc = cssm_build_model(&same, desc, true);
    if (rc) { const std::string keep = cssm_last_error(); return fail(rc, "cssm_fleet_if2: desc is not of the fleet's model structure (%s)", keep.c_str()); }
  }
  HIP_TRY(hipSetDevice(f->device));
  const size_t nt = n_theta, R = (size_t)off[S], RB = CSSM_FLEET_IF2_REC_BYTES(d);
  // staged upload: offsets | seeds | rw_sd | cool | records
  const size_t o_seeds = ((size_t)S + 1u) * 8u, o_sd = o_seeds + (size_t)S * 8u, o_cool = o_sd + nt * 8u, o_recs = o_cool + (size_t)n_iters * 8u;
  std::vector<unsigned char> stage(o_recs + R * RB);
  memcpy(stage.data(), off, ((size_t)S + 1u) * 8u);
  memcpy(stage.data() + o_seeds, seeds, (size_t)S * 8u);
  memcpy(stage.data() + o_sd, rw_sd, nt * 8u);
  memcpy(stage.data() + o_cool, cool.data(), (size_t)n_iters * 8u);
  fleet_if2_recs(f, probe, off, t, y, has_obs, stage.data() + o_recs);
  CssmTemps tmp;
  unsigned char* d_stage = nullptr;
  double *d_swarm = nullptr, *d_theta = nullptr, *d_x = nullptr, *d_mean = nullptr, *d_ll = nullptr, *d_ll_t = nullptr;
  int32_t* d_ess_t = nullptr; uint32_t* d_anc = nullptr; FleetIf2Series* d_ser = nullptr;
  const size_t sw_bytes = (size_t)S * nt * n * 8u, x_bytes = (size_t)S * 2u * d * n * 8u, mean_bytes = (size_t)S * n_iters * nt * 8u;
  HIP_ALLOC(tmp, d_stage, stage.size());
  HIP_ALLOC(tmp, d_swarm, sw_bytes);
  HIP_ALLOC(tmp, d_theta, 2u * sw_bytes);
  HIP_ALLOC(tmp, d_x, x_bytes);
  HIP_ALLOC(tmp, d_mean, mean_bytes);
  HIP_ALLOC(tmp, d_ll, (size_t)S * n_iters * 8u);
  HIP_ALLOC(tmp, d_ser, (size_t)S * sizeof(FleetIf2Series));
  if (ll_t && R) HIP_ALLOC(tmp, d_ll_t, R * 8u);
  if (ess_t && R) HIP_ALLOC(tmp, d_ess_t, R * 4u);
  if (anc_out) HIP_ALLOC(tmp, d_anc, (size_t)S * n * 4u);
  hipEvent_t e0 = nullptr, e1 = nullptr;
  HIP_TRY(tmp.event(e0)); HIP_TRY(tmp.event(e1));
  HIP_TRY(hipMemcpyAsync(d_stage, stage.data(), stage.size(), hipMemcpyHostToDevice, f->stream));
  {   // the starting swarm: the caller's, or every particle of series k at theta0[k]
    std::vector<double> sw;
    const double* src = swarm0;
    if (!swarm0) {
      sw.resize((size_t)S * nt * n);
      for (size_t k = 0; k < S; ++k)
        for (size_t j = 0; j < nt; ++j) std::fill_n(sw.data() + (k * nt + j) * n, n, theta0[k * nt + j]);
      src = sw.data();
    }
    HIP_TRY(hipMemcpyAsync(d_swarm, src, sw_bytes, hipMemcpyHostToDevice, f->stream));
    HIP_TRY(hipStreamSynchronize(f->stream));   // (stage and sw are pageable)
  }
  HIP_TRY(hipMemsetAsync(d_ser, 0, (size_t)S * sizeof(FleetIf2Series), f->stream));
  HIP_TRY(hipMemsetAsync(d_mean, 0xff, mean_bytes, f->stream));   // (rows no iteration writes are not read back)
  HIP_TRY(hipMemsetAsync(d_ll, 0xff, (size_t)S * n_iters * 8u, f->stream));
  if (d_ll_t) HIP_TRY(hipMemsetAsync(d_ll_t, 0xff, R * 8u, f->stream));
  if (d_ess_t) HIP_TRY(hipMemsetAsync(d_ess_t, 0xff, R * 4u, f->stream));
  FleetIf2Launch l{};
  l.args.n = n; l.args.n_theta = (uint32_t)nt; l.args.n_iters = n_iters; l.args.first_iter = first_iter;
  l.args.swarm = d_swarm; l.args.theta = d_theta; l.args.x = d_x; l.args.ser = d_ser;
  l.args.off = reinterpret_cast<const unsigned long long*>(d_stage);
  l.args.seeds = reinterpret_cast<const unsigned long long*>(d_stage + o_seeds);
  l.args.rw_sd = reinterpret_cast<const double*>(d_stage + o_sd);
  l.args.cool = reinterpret_cast<const double*>(d_stage + o_cool);
  l.args.recs = d_stage + o_recs;
  l.args.theta_mean = d_mean; l.args.ll = d_ll; l.args.ll_t = d_ll_t; l.args.ess_t = d_ess_t;
  l.args.logtab = f->logtab.at<const double>();
  l.args.df = (double)probe.obs_df; l.args.mk = f->base.mk; l.args.map = map;
  l.n_series = S; l.d = d; l.threads = f->threads; l.lds = f->lds; l.stream = f->stream;
  const uint32_t per = (iters_per_launch == 0u || iters_per_launch > n_iters) ? n_iters : iters_per_launch;
  HIP_TRY(hipEventRecord(e0, f->stream));
  for (uint32_t it0 = 0; it0 < n_iters && R; it0 += per) {      // (the result does not depend on the split: a launch leaves the swarm in HBM)
    l.args.it0 = it0; l.args.it1 = std::min(n_iters, it0 + per);
    l.args.anc_out = (l.args.it1 == n_iters) ? d_anc : nullptr;
    const int hrc = cssm_fleet_if2_launch(l);
    if (hrc) return fail(CSSM_EHIP, "k_fleet_if2: %s", hipGetErrorString((hipError_t)hrc));
  }
  HIP_TRY(hipEventRecord(e1, f->stream));
  std::vector<double> h_mean((size_t)S * n_iters * nt), h_ll((size_t)S * n_iters), h_x(x_out ? x_bytes / 8u : 0u);
  std::vector<FleetIf2Series> h_ser(S);
  HIP_TRY(hipMemcpyAsync(h_mean.data(), d_mean, mean_bytes, hipMemcpyDeviceToHost, f->stream));
  HIP_TRY(hipMemcpyAsync(h_ll.data(), d_ll, h_ll.size() * 8u, hipMemcpyDeviceToHost, f->stream));
  HIP_TRY(hipMemcpyAsync(h_ser.data(), d_ser, (size_t)S * sizeof(FleetIf2Series), hipMemcpyDeviceToHost, f->stream));
  if (swarm_out) HIP_TRY(hipMemcpyAsync(swarm_out, d_swarm, sw_bytes, hipMemcpyDeviceToHost, f->stream));
  if (d_ll_t) HIP_TRY(hipMemcpyAsync(ll_t, d_ll_t, R * 8u, hipMemcpyDeviceToHost, f->stream));
  if (d_ess_t) HIP_TRY(hipMemcpyAsync(ess_t, d_ess_t, R * 4u, hipMemcpyDeviceToHost, f->stream));
  if (x_out) HIP_TRY(hipMemcpyAsync(h_x.data(), d_x, x_bytes, hipMemcpyDeviceToHost, f->stream));
  if (anc_out) HIP_TRY(hipMemcpyAsync(anc_out, d_anc, (size_t)S * n * 4u, hipMemcpyDeviceToHost, f->stream));
  HIP_TRY(hipStreamSynchronize(f->stream));
  float ms = 0.f;
  f->ms_if2 = (hipEventElapsedTime(&ms, e0, e1) == hipSuccess) ? (double)ms : -1.0;
  for (uint32_t k = 0; k < S; ++k) {
    const size_t a = (size_t)off[k], T = (size_t)off[k + 1] - a;
    const bool failed = T != 0 && h_ser[k].err != 0u;
    const uint32_t done = T == 0 ? 0u : (failed ? h_ser[k].fail_iter : n_iters);   // the iterations whose rows stand
    rc_out[k] = failed ? CSSM_ENONFINITE : CSSM_OK;
    for (uint32_t m = 0; m < n_iters; ++m) {
      const size_t row = (size_t)k * n_iters + m;
      ll[row] = m < done ? h_ll[row] : cssm_nan();
      for (size_t j = 0; j < nt; ++j) theta_mean[row * nt + j] = m < done ? h_mean[row * nt + j] : cssm_nan();
    }
    const bool whole = T != 0 && !failed;                        // the last iteration's diagnostics exist
    if (ll_t && !whole) std::fill(ll_t + a, ll_t + a + T, cssm_nan());
    if (ess_t && !whole) std::fill(ess_t + a, ess_t + a + T, -1);
    if (anc_out && !whole) std::fill(anc_out + (size_t)k * n, anc_out + ((size_t)k + 1u) * n, 0xffffffffu);
    if (x_out) {                                                 // the cloud the last record proposed: record T - 1 wrote buffer T & 1
      double* dst = x_out + (size_t)k * d * n;
      if (whole) memcpy(dst, h_x.data() + ((size_t)k * 2u + (T & 1u)) * d * n, (size_t)d * n * 8u);
      else std::fill(dst, dst + (size_t)d * n, cssm_nan());
    }
  }
  return CSSM_OK;
}

extern "C" int cssm_fleet_if2_last_ms(cssm_fleet* f, double* ms) {
  if (!f || !ms) return fail(CSSM_EINVAL_ARG, "null argument");
  if (f->ms_if2 < 0.0) return fail(CSSM_ESTATE, "no search has run on this fleet (cssm_fleet_if2 first)");
  *ms = f->ms_if2;
  return CSSM_OK;
}

// ParticleMetropolisHastings with the reference's prior argument and Parameters.perturbMvn (model/PMMH.scala:32,68-81; model/
// Parameters.scala:111-123) -- S whole chains, one workgroup each, every iteration and record of a chain inside k_fleet_pmmh
// (cssm_fleet_pmmh.hip).  The arithmetic is the contract's (include/cssm_numerics.h, "PMMH chains on the device").  The fleet lends its
// device, stream, contract table, N and structure; the chains, the states and the records live in buffers of the call.
static int fleet_pmmh_chol_check(const char* call, const double* L, size_t nt, size_t which) {
  for (size_t i = 0; i < nt; ++i)
    for (size_t j = 0; j < nt; ++j) {
      const double v = L[i * nt + j];
      if (!std::isfinite(v)) return fail(CSSM_EINVAL_ARG, "%s: chol %zu [%zu][%zu] is not finite", call, which, i, j);
      if (j > i && v != 0.0)
        return fail(CSSM_EINVAL_ARG, "%s: chol %zu [%zu][%zu] = %g lies above the diagonal (a lower-triangular factor, row-major)", call, which, i, j, v);
    }
  return CSSM_OK;
}
// the n_theta priors as the kernel reads them (null: all flat), or the refusal of one
static int fleet_pmmh_priors(const char* call, const cssm_prior* priors, size_t nt, std::vector<cssm_prior>& pri) {
  pri.resize(nt);
  for (size_t j = 0; j < nt; ++j) {
    cssm_prior p{};
    if (priors) p = priors[j];
    p.pad_ = 0;
    if (p.kind == CSSM_PRIOR_FLAT) { p.a = 0.0; p.b = 0.0; }
    else if (p.kind == CSSM_PRIOR_NORMAL) {
      if (!std::isfinite(p.a) || !std::isfinite(p.b) || !(p.b > 0.0))
        return fail(CSSM_EINVAL_ARG, "%s: priors[%zu]: a NORMAL prior needs a finite mean and a finite sd > 0 (got %g, %g)", call, j, p.a, p.b);
    } else if (p.kind == CSSM_PRIOR_UNIFORM) {
      if (!(p.a <= p.b)) return fail(CSSM_EINVAL_ARG, "%s: priors[%zu]: a UNIFORM prior needs a <= b (got %g, %g)", call, j, p.a, p.b);
    } else {
      return fail(CSSM_EINVAL_ARG, "%s: priors[%zu]: unknown kind %d", call, j, (int)p.kind);
    }
    pri[j] = p;
  }
  return CSSM_OK;
}
// the chains as they start, [S] rows of cur_ll | lp_cur | cur | cur_state, or the refusal of a theta0 row outside the prior's support
static int fleet_pmmh_start(const char* call, uint32_t S, size_t nt, int d, const std::vector<cssm_prior>& pri, const double* theta0, const double* ll0,
                            const double* state0, std::vector<double>& chain) {
  const size_t CR = CSSM_FLEET_PMMH_ROW(nt, d);
  chain.assign((size_t)S * CR, 0.0);
  for (uint32_t k = 0; k < S; ++k) {
    double* row = chain.data() + (size_t)k * CR;
    const double* th = theta0 + (size_t)k * nt;
    double lp = 0.0;
    for (size_t j = 0; j < nt; ++j)
      if (pri[j].kind != CSSM_PRIOR_FLAT) lp = lp + cssm_prior_term(pri[j].kind, pri[j].a, pri[j].b, th[j]);
    if (!(lp > -cssm_inf())) return fail(CSSM_EINVAL_ARG, "%s: chain %u: theta0 lies outside the prior's support (its log-prior is %g)", call, k, lp);
    row[0] = ll0 ? ll0[k] : -1e99;
    row[1] = lp;
    memcpy(row + 2, th, nt * 8u);
    for (int c = 0; c < d; ++c) row[2 + nt + c] = state0 ? state0[(size_t)k * d + c] : 0.0;
  }
  return CSSM_OK;
}
// what a chains call returns per chain: its status and counters; a chain without records ran no block, its rows read NaN
static void fleet_pmmh_finish(uint32_t S, size_t nt, int d, uint32_t n_iters, const uint64_t* off, const std::vector<uint32_t>& h_count, double* ll,
                              double* theta, int32_t* accepted, double* last_state, uint32_t* diag_out, int* rc_out) {
  for (uint32_t k = 0; k < S; ++k) {
    const bool ran = off[k + 1] > off[k];
    rc_out[k] = ran ? CSSM_OK : CSSM_EINVAL_ARG;
    if (diag_out) { diag_out[2u * k] = ran ? h_count[4u * k + 1u] : 0u; diag_out[2u * k + 1u] = ran ? h_count[4u * k + 2u] : 0u; }
    if (ran) continue;
    const size_t r0 = (size_t)k * n_iters;
    std::fill(ll + r0, ll + r0 + n_iters, cssm_nan());
    std::fill(theta + r0 * nt, theta + (r0 + n_iters) * nt, cssm_nan());
    std::fill(last_state + r0 * d, last_state + (r0 + n_iters) * d, cssm_nan());
    std::fill(accepted + r0, accepted + r0 + n_iters, -1);
  }
}
extern "C" int cssm_fleet_pmmh_chains(cssm_fleet* f, const cssm_model_desc* desc, const double* theta0, size_t n_theta, const double* chol,
                                      int chol_per_chain, const void* priors_, const double* ll0, const double* state0, uint32_t first_iter,
                                      uint32_t n_iters, uint32_t iters_per_launch, const uint64_t* seeds, const uint64_t* off, const double* t,
                                      const double* y, const uint8_t* has_obs, double* ll, double* theta, int32_t* accepted, double* last_state,
                                      uint32_t* diag_out, int* rc_out) {
  if (!desc || !theta0 || !chol || !seeds || !off) return fail(CSSM_EINVAL_ARG, "cssm_fleet_pmmh_chains: null argument (desc, theta0, chol, seeds, off)");
  const cssm_prior* priors = static_cast<const cssm_prior*>(priors_);
  if (!ll || !theta || !accepted || !last_state || !rc_out)
    return fail(CSSM_EINVAL_ARG, "cssm_fleet_pmmh_chains: null output (ll, theta, accepted, last_state, rc_out)");
  if (off[0] != 0) return fail(CSSM_EINVAL_ARG, "off[0] must be 0");
  if (!t || !y) return fail(CSSM_EINVAL_ARG, "null data");
  HostModel probe;
  int rc = cssm_build_model(&probe, desc, false);
  if (rc) return rc;
  if (probe.obs_kind == CSSM_OBS_LGCP)
    return fail(CSSM_EINVAL_DESC, "cssm_fleet_pmmh_chains: the LGCP observation model (sub-stepped events) is not served; " FLEET_PMMH_SERVED);
  If2Map map;
  if ((rc = cssm_if2_map_build(desc, &map))) return rc;
  if ((size_t)map.n_theta != n_theta)
    return fail(CSSM_EINVAL_ARG, "cssm_fleet_pmmh_chains: n_theta = %zu, the descriptor flattens to %d (cssm_desc_flatten)", n_theta, (int)map.n_theta);
  const size_t nt = n_theta;
  if ((rc = fleet_pmmh_chol_check("cssm_fleet_pmmh_chains", chol, nt, 0))) return rc;
  std::vector<cssm_prior> pri;
  if ((rc = fleet_pmmh_priors("cssm_fleet_pmmh_chains", priors, nt, pri))) return rc;
  if (n_iters < 1u || n_iters > 1000000u) return fail(CSSM_EINVAL_ARG, "cssm_fleet_pmmh_chains: n_iters must be in [1, 1000000] (got %u)", n_iters);
  if ((uint64_t)first_iter + n_iters > (1ull << 31)) return fail(CSSM_EINVAL_ARG, "cssm_fleet_pmmh_chains: first_iter + n_iters must not exceed 2^31");
  FLEET_LGCP_REFUSE(f, "cssm_fleet_pmmh_chains", FLEET_PMMH_SERVED);
  if (!f) return fail(CSSM_EINVAL_ARG, "null fleet");
  const uint32_t S = f->S, n = f->n;
  const int d = f->d;
  for (uint32_t k = 0; k < S; ++k) {
    if ((rc = fleet_off_step("off", off, k))) return rc;
    if (off[k + 1] - off[k] > 0xfffffffeull) return fail(CSSM_EINVAL_ARG, "series %u: too many records", k);
  }
  {   // the structure must be the fleet's
    HostModel same = f->base;
    rc = cssm_build_model(&same, desc, true);
    if (rc) { const std::string keep = cssm_last_error(); return fail(rc, "cssm_fleet_pmmh_chains: desc is not of the fleet's model structure (%s)", keep.c_str()); }
  }
  for (uint32_t k = 1; k < S && chol_per_chain; ++k)
    if ((rc = fleet_pmmh_chol_check("cssm_fleet_pmmh_chains", chol + (size_t)k * nt * nt, nt, k))) return rc;
  std::vector<double> chain;
  if ((rc = fleet_pmmh_start("cssm_fleet_pmmh_chains", S, nt, d, pri, theta0, ll0, state0, chain))) return rc;
  HIP_TRY(hipSetDevice(f->device));
  const size_t R = (size_t)off[S], RB = CSSM_FLEET_IF2_REC_BYTES(d);
  const size_t n_chol = chol_per_chain ? (size_t)S : (size_t)1;
  // staged upload: offsets | seeds | chol | priors | chains | records
  const size_t o_seeds = ((size_t)S + 1u) * 8u, o_chol = o_seeds + (size_t)S * 8u, o_pri = o_chol + n_chol * nt * nt * 8u,
               o_chain = o_pri + nt * sizeof(cssm_prior), o_recs = o_chain + chain.size() * 8u;
  std::vector<unsigned char> stage(o_recs + R * RB);
  memcpy(stage.data(), off, ((size_t)S + 1u) * 8u);
  memcpy(stage.data() + o_seeds, seeds, (size_t)S * 8u);
  memcpy(stage.data() + o_chol, chol, n_chol * nt * nt * 8u);
  memcpy(stage.data() + o_pri, pri.data(), nt * sizeof(cssm_prior));
  memcpy(stage.data() + o_chain, chain.data(), chain.size() * 8u);
  fleet_if2_recs(f, probe, off, t, y, has_obs, stage.data() + o_recs);
  CssmTemps tmp;
  unsigned char* d_stage = nullptr;
  double *d_x = nullptr, *d_ll = nullptr, *d_theta = nullptr, *d_last = nullptr;
  int32_t* d_acc = nullptr; uint32_t* d_count = nullptr;
  const size_t rows = (size_t)S * n_iters;
  HIP_ALLOC(tmp, d_stage, stage.size());
  HIP_ALLOC(tmp, d_x, (size_t)S * 2u * d * n * 8u);
  HIP_ALLOC(tmp, d_ll, rows * 8u);
  HIP_ALLOC(tmp, d_theta, rows * nt * 8u);
  HIP_ALLOC(tmp, d_last, rows * d * 8u);
  HIP_ALLOC(tmp, d_acc, rows * 4u);
  HIP_ALLOC(tmp, d_count, (size_t)S * 16u);
  hipEvent_t e0 = nullptr, e1 = nullptr;
  HIP_TRY(tmp.event(e0)); HIP_TRY(tmp.event(e1));
  HIP_TRY(hipMemcpyAsync(d_stage, stage.data(), stage.size(), hipMemcpyHostToDevice, f->stream));
  HIP_TRY(hipStreamSynchronize(f->stream));   // (stage is pageable)
  HIP_TRY(hipMemsetAsync(d_count, 0, (size_t)S * 16u, f->stream));
  FleetPmmhLaunch l{};
  l.args.n = n; l.args.n_theta = (uint32_t)nt; l.args.n_iters = n_iters; l.args.first_iter = first_iter;
  l.args.chol_stride = chol_per_chain ? (uint32_t)(nt * nt) : 0u;
  l.args.x = d_x; l.args.chain = reinterpret_cast<double*>(d_stage + o_chain); l.args.count = d_count;
  l.args.off = reinterpret_cast<const unsigned long long*>(d_stage);
  l.args.seeds = reinterpret_cast<const unsigned long long*>(d_stage + o_seeds);
  l.args.chol = reinterpret_cast<const double*>(d_stage + o_chol);
  l.args.priors = reinterpret_cast<const cssm_prior*>(d_stage + o_pri);
  l.args.recs = d_stage + o_recs;
  l.args.ll = d_ll; l.args.theta = d_theta; l.args.accepted = d_acc; l.args.last = d_last;
  l.args.logtab = f->logtab.at<const double>();
  l.args.df = (double)probe.obs_df; l.args.mk = f->base.mk; l.args.map = map;
  l.n_series = S; l.d = d; l.threads = f->threads; l.lds = f->lds; l.stream = f->stream;
  const uint32_t per = (iters_per_launch == 0u || iters_per_launch > n_iters) ? n_iters : iters_per_launch;
  HIP_TRY(hipEventRecord(e0, f->stream));
  for (uint32_t it0 = 0; it0 < n_iters && R; it0 += per) {      // (the result does not depend on the split: a launch leaves the chains in HBM)
    l.args.it0 = it0; l.args.it1 = std::min(n_iters, it0 + per);
    const int hrc = cssm_fleet_pmmh_launch(l);
    if (hrc) return fail(CSSM_EHIP, "k_fleet_pmmh: %s", hipGetErrorString((hipError_t)hrc));
  }
  HIP_TRY(hipEventRecord(e1, f->stream));
  std::vector<uint32_t> h_count((size_t)S * 4u);
  HIP_TRY(hipMemcpyAsync(ll, d_ll, rows * 8u, hipMemcpyDeviceToHost, f->stream));
  HIP_TRY(hipMemcpyAsync(theta, d_theta, rows * nt * 8u, hipMemcpyDeviceToHost, f->stream));
  HIP_TRY(hipMemcpyAsync(last_state, d_last, rows * d * 8u, hipMemcpyDeviceToHost, f->stream));
  HIP_TRY(hipMemcpyAsync(accepted, d_acc, rows * 4u, hipMemcpyDeviceToHost, f->stream));
  HIP_TRY(hipMemcpyAsync(h_count.data(), d_count, (size_t)S * 16u, hipMemcpyDeviceToHost, f->stream));
  HIP_TRY(hipStreamSynchronize(f->stream));
  float ms = 0.f;
  f->ms_pmmh_chains = (hipEventElapsedTime(&ms, e0, e1) == hipSuccess) ? (double)ms : -1.0;
  fleet_pmmh_finish(S, nt, d, n_iters, off, h_count, ll, theta, accepted, last_state, diag_out, rc_out);
  return CSSM_OK;
}

extern "C" int cssm_fleet_pmmh_chains_last_ms(cssm_fleet* f, double* ms) {
  if (!f || !ms) return fail(CSSM_EINVAL_ARG, "null argument");
  if (f->ms_pmmh_chains < 0.0) return fail(CSSM_ESTATE, "no chains have run on this fleet (cssm_fleet_pmmh_chains first)");
  *ms = f->ms_pmmh_chains;
  return CSSM_OK;
}

// ParticleMetropolisHastings over FilterLgcp (model/ParticleFilter.scala:169-227) -- cssm_fleet_pmmh_chains for an LGCP fleet, asked for by
// name as cssm_fleet_create_lgcp is: S whole chains, one workgroup each, every iteration and event of a chain inside k_fleet_pmmh_lgcp
// (cssm_fleet_pmmh_lgcp.hip).  The arithmetic is the contract's (include/cssm_numerics.h, "PMMH chains on the device: LGCP").  The fleet
// lends its device, stream, contract table, N and structure; the chains, the states, the records and the sub-step table live in buffers
// of the call.
//
// The record of the event at t behind t_prev that does not depend on the parameters: cssm_build_rec's n_sub, dt and F(t), and the rows of
// cssm_build_fsub_table appended to `tab` (fsub_off counts from `tab_base` doubles before it), as fleet_pack_rec_lgcp takes them.
static int fleet_pmmh_lgcp_pack(const HostModel& m, double t_prev, double t, uint32_t step, unsigned char* dst, std::vector<double>& tab, size_t tab_base) {
  StepRec r;
  cssm_build_rec(&m, t_prev, t, 0.0, 1, step, &r);
  const int rc = cssm_build_fsub_table(&m, &r, 0, 1, tab);
  if (rc) return rc;
  FleetPmmhLgcpRec h;
  h.dt = r.dt; h.n_sub = r.n_sub; h.step = r.step; h.fsub_off = (uint32_t)(tab_base + r.fsub_off); h.pad_ = 0u;
  memcpy(dst, &h, sizeof h);
  memcpy(dst + sizeof h, r.fco, (size_t)m.d * 8u);
  return CSSM_OK;
}
#define FLEET_PMMH_LGCP "cssm_fleet_pmmh_chains_lgcp"
extern "C" int cssm_fleet_pmmh_chains_lgcp(cssm_fleet* f, const cssm_model_desc* desc, const double* theta0, size_t n_theta, const double* chol,
                                           int chol_per_chain, const void* priors_, const double* ll0, const double* state0, uint32_t first_iter,
                                           uint32_t n_iters, uint32_t iters_per_launch, const uint64_t* seeds, const uint64_t* off, const double* t,
                                           double* ll, double* theta, int32_t* accepted, double* last_state, uint32_t* diag_out, int* rc_out) {
  if (!desc || !theta0 || !chol || !seeds || !off) return fail(CSSM_EINVAL_ARG, FLEET_PMMH_LGCP ": null argument (desc, theta0, chol, seeds, off)");
  const cssm_prior* priors = static_cast<const cssm_prior*>(priors_);
  if (!ll || !theta || !accepted || !last_state || !rc_out)
    return fail(CSSM_EINVAL_ARG, FLEET_PMMH_LGCP ": null output (ll, theta, accepted, last_state, rc_out)");
  if (off[0] != 0) return fail(CSSM_EINVAL_ARG, "off[0] must be 0");
  if (!t) return fail(CSSM_EINVAL_ARG, "null data");
  HostModel probe;
  int rc = cssm_build_model(&probe, desc, false);
  if (rc) return rc;
  if (probe.obs_kind != CSSM_OBS_LGCP)
    return fail(CSSM_EINVAL_DESC, FLEET_PMMH_LGCP " runs chains over LGCP event streams (obs_kind %d given): cssm_fleet_pmmh_chains serves every other "
                                  "observation model", probe.obs_kind);
  If2Map map;
  if ((rc = cssm_if2_map_build(desc, &map))) return rc;
  if ((size_t)map.n_theta != n_theta)
    return fail(CSSM_EINVAL_ARG, FLEET_PMMH_LGCP ": n_theta = %zu, the descriptor flattens to %d (cssm_desc_flatten)", n_theta, (int)map.n_theta);
  const size_t nt = n_theta;
  if ((rc = fleet_pmmh_chol_check(FLEET_PMMH_LGCP, chol, nt, 0))) return rc;
  std::vector<cssm_prior> pri;
  if ((rc = fleet_pmmh_priors(FLEET_PMMH_LGCP, priors, nt, pri))) return rc;
  if (n_iters < 1u || n_iters > 1000000u) return fail(CSSM_EINVAL_ARG, FLEET_PMMH_LGCP ": n_iters must be in [1, 1000000] (got %u)", n_iters);
  if ((uint64_t)first_iter + n_iters > (1ull << 31)) return fail(CSSM_EINVAL_ARG, FLEET_PMMH_LGCP ": first_iter + n_iters must not exceed 2^31");
  if (!f) return fail(CSSM_EINVAL_ARG, "null fleet");
  if (!f->lgcp)
    return fail(CSSM_EINVAL_ARG, FLEET_PMMH_LGCP ": the fleet was not made by cssm_fleet_create_lgcp; cssm_fleet_pmmh_chains runs the chains of every "
                                 "other fleet");
  const uint32_t S = f->S, n = f->n;
  const int d = f->d;
  for (uint32_t k = 0; k < S; ++k) {
    if ((rc = fleet_off_step("off", off, k))) return rc;
    if (off[k + 1] - off[k] > 0xfffffffeull) return fail(CSSM_EINVAL_ARG, "series %u: too many records", k);
  }
  {   // the structure, the precision with it, must be the fleet's
    HostModel same = f->base;
    rc = cssm_build_model(&same, desc, true);
    if (rc) { const std::string keep = cssm_last_error(); return fail(rc, FLEET_PMMH_LGCP ": desc is not of the fleet's model structure (%s)", keep.c_str()); }
  }
  for (uint32_t k = 1; k < S && chol_per_chain; ++k)
    if ((rc = fleet_pmmh_chol_check(FLEET_PMMH_LGCP, chol + (size_t)k * nt * nt, nt, k))) return rc;
  std::vector<double> chain;
  if ((rc = fleet_pmmh_start(FLEET_PMMH_LGCP, S, nt, d, pri, theta0, ll0, state0, chain))) return rc;
  HIP_TRY(hipSetDevice(f->device));
  const size_t R = (size_t)off[S], RB = CSSM_FLEET_PMMH_LGCP_REC_BYTES(d);
  const size_t n_chol = chol_per_chain ? (size_t)S : (size_t)1;
  auto t_min = [&](size_t a, size_t b) {                        // data.minBy(_.t).t: where a fresh series' first increment starts
    double m = t[a];
    for (size_t s = a + 1; s < b; ++s) m = (t[s] < m) ? t[s] : m;
    return m;
  };
  // (f depends on time) where chain k's rows start in the call's sub-step table (doubles): theta-independent, uploaded once
  std::vector<size_t> toff((size_t)S + 1u, 0);
  if (f->base.lgcp_tdep) {
    fleet_parallel(S, R, [&](size_t lo, size_t hi) {
      for (size_t k = lo; k < hi; ++k) {
        const size_t a = (size_t)off[k], b = (size_t)off[k + 1];
        if (b > a) toff[k + 1] = fleet_lgcp_rows(f->base, t_min(a, b), t + a, b - a);
      }
    });
    for (uint32_t k = 0; k < S; ++k) toff[k + 1] += toff[k];
    if ((rc = fleet_lgcp_table_fits(toff[S]))) return rc;
  }
  // staged upload: offsets | seeds | chol | priors | chains | records | sub-step table
  const size_t o_seeds = ((size_t)S + 1u) * 8u, o_chol = o_seeds + (size_t)S * 8u, o_pri = o_chol + n_chol * nt * nt * 8u,
               o_chain = o_pri + nt * sizeof(cssm_prior), o_recs = o_chain + chain.size() * 8u, o_fsub = o_recs + fleet_pad8(R * RB);
  std::vector<unsigned char> stage(o_fsub + toff[S] * 8u);
  memcpy(stage.data(), off, ((size_t)S + 1u) * 8u);
  memcpy(stage.data() + o_seeds, seeds, (size_t)S * 8u);
  memcpy(stage.data() + o_chol, chol, n_chol * nt * nt * 8u);
  memcpy(stage.data() + o_pri, pri.data(), nt * sizeof(cssm_prior));
  memcpy(stage.data() + o_chain, chain.data(), chain.size() * 8u);
  std::atomic<int> pack_rc{CSSM_OK};
  fleet_parallel(S, R, [&](size_t lo, size_t hi) {
    for (size_t k = lo; k < hi; ++k) {
      const size_t a = (size_t)off[k], b = (size_t)off[k + 1];
      if (b == a) continue;
      std::vector<double> tab;
      double tp = t_min(a, b);
      for (size_t s = a; s < b; ++s) {
        const int prc = fleet_pmmh_lgcp_pack(f->base, tp, t[s], (uint32_t)(s - a), stage.data() + o_recs + s * RB, tab, toff[k]);
        if (prc) pack_rc = prc;
        tp = t[s];
      }
      if (tab.size() != toff[k + 1] - toff[k]) pack_rc = CSSM_ENOMEM;
      else if (!tab.empty()) memcpy(stage.data() + o_fsub + toff[k] * 8u, tab.data(), tab.size() * 8u);
    }
  });
  if (pack_rc) return fail(pack_rc, FLEET_PMMH_LGCP ": the sub-step table of the call could not be built");
  CssmTemps tmp;
  unsigned char* d_stage = nullptr;
  double *d_x = nullptr, *d_ll = nullptr, *d_theta = nullptr, *d_last = nullptr;
  int32_t* d_acc = nullptr; uint32_t* d_count = nullptr;
  const size_t rows = (size_t)S * n_iters;
  HIP_ALLOC(tmp, d_stage, stage.size());
  HIP_ALLOC(tmp, d_x, (size_t)S * 2u * d * n * 8u);
  HIP_ALLOC(tmp, d_ll, rows * 8u);
  HIP_ALLOC(tmp, d_theta, rows * nt * 8u);
  HIP_ALLOC(tmp, d_last, rows * d * 8u);
  HIP_ALLOC(tmp, d_acc, rows * 4u);
  HIP_ALLOC(tmp, d_count, (size_t)S * 16u);
  hipEvent_t e0 = nullptr, e1 = nullptr;
  HIP_TRY(tmp.event(e0)); HIP_TRY(tmp.event(e1));
  HIP_TRY(hipMemcpyAsync(d_stage, stage.data(), stage.size(), hipMemcpyHostToDevice, f->stream));
  HIP_TRY(hipStreamSynchronize(f->stream));   // (stage is pageable)
  HIP_TRY(hipMemsetAsync(d_count, 0, (size_t)S * 16u, f->stream));
  FleetPmmhLgcpLaunch l{};
  l.args.n = n; l.args.n_theta = (uint32_t)nt; l.args.n_iters = n_iters; l.args.first_iter = first_iter;
  l.args.chol_stride = chol_per_chain ? (uint32_t)(nt * nt) : 0u;
  l.args.delta = std::pow(10.0, -f->base.precision);            // cssm_build_rec's expression: the sub-step of every record with n_sub > 0
  l.args.x = d_x; l.args.chain = reinterpret_cast<double*>(d_stage + o_chain); l.args.count = d_count;
  l.args.off = reinterpret_cast<const unsigned long long*>(d_stage);
  l.args.seeds = reinterpret_cast<const unsigned long long*>(d_stage + o_seeds);
  l.args.chol = reinterpret_cast<const double*>(d_stage + o_chol);
  l.args.priors = reinterpret_cast<const cssm_prior*>(d_stage + o_pri);
  l.args.recs = d_stage + o_recs;
  l.args.fsub = f->base.lgcp_tdep ? reinterpret_cast<const double*>(d_stage + o_fsub) : nullptr;   // (otherwise null: f is every record's own)
  l.args.ll = d_ll; l.args.theta = d_theta; l.args.accepted = d_acc; l.args.last = d_last;
  l.args.logtab = f->logtab.at<const double>();
  l.args.mk = f->base.mk; l.args.map = map;
  l.n_series = S; l.d = d; l.threads = f->threads; l.lds = f->lds; l.stream = f->stream;
  const uint32_t per = (iters_per_launch == 0u || iters_per_launch > n_iters) ? n_iters : iters_per_launch;
  HIP_TRY(hipEventRecord(e0, f->stream));
  for (uint32_t it0 = 0; it0 < n_iters && R; it0 += per) {      // (the result does not depend on the split: a launch leaves the chains in HBM)
    l.args.it0 = it0; l.args.it1 = std::min(n_iters, it0 + per);
    const int hrc = cssm_fleet_pmmh_lgcp_launch(l);
    if (hrc) return fail(CSSM_EHIP, "k_fleet_pmmh_lgcp: %s", hipGetErrorString((hipError_t)hrc));
  }
  HIP_TRY(hipEventRecord(e1, f->stream));
  std::vector<uint32_t> h_count((size_t)S * 4u);
  HIP_TRY(hipMemcpyAsync(ll, d_ll, rows * 8u, hipMemcpyDeviceToHost, f->stream));
  HIP_TRY(hipMemcpyAsync(theta, d_theta, rows * nt * 8u, hipMemcpyDeviceToHost, f->stream));
  HIP_TRY(hipMemcpyAsync(last_state, d_last, rows * d * 8u, hipMemcpyDeviceToHost, f->stream));
  HIP_TRY(hipMemcpyAsync(accepted, d_acc, rows * 4u, hipMemcpyDeviceToHost, f->stream));
  HIP_TRY(hipMemcpyAsync(h_count.data(), d_count, (size_t)S * 16u, hipMemcpyDeviceToHost, f->stream));
  HIP_TRY(hipStreamSynchronize(f->stream));
  float ms = 0.f;
  f->ms_pmmh_lgcp = (hipEventElapsedTime(&ms, e0, e1) == hipSuccess) ? (double)ms : -1.0;
  fleet_pmmh_finish(S, nt, d, n_iters, off, h_count, ll, theta, accepted, last_state, diag_out, rc_out);
  return CSSM_OK;
}

extern "C" int cssm_fleet_pmmh_chains_lgcp_last_ms(cssm_fleet* f, double* ms) {
  if (!f || !ms) return fail(CSSM_EINVAL_ARG, "null argument");
  if (f->ms_pmmh_lgcp < 0.0) return fail(CSSM_ESTATE, "no chains have run on this fleet (" FLEET_PMMH_LGCP " first)");
  *ms = f->ms_pmmh_lgcp;
  return CSSM_OK;
}

// The theta-independent record of one event as cssm_fleet_pmmh_chains_lgcp uploads it, and the rows of the sub-step table it brings
// (fsub_off = 0: the table is this event's own).  No device.
extern "C" int cssm_fleet_pmmh_lgcp_pack_record(const cssm_model_desc* desc, double t_prev, double t, uint32_t step, unsigned char* out, size_t cap,
                                                size_t* bytes, double* fsub_out, size_t fsub_cap, size_t* fsub_count) {
  if (!out || !bytes || !fsub_count) return fail(CSSM_EINVAL_ARG, "null argument");
  HostModel m;
  const int rc = cssm_build_model(&m, desc, false);
  if (rc) return rc;
  if (m.obs_kind != CSSM_OBS_LGCP)
    return fail(CSSM_EINVAL_DESC, "cssm_fleet_pmmh_lgcp_pack_record packs LGCP events (obs_kind %d given)", m.obs_kind);
  m.n_global = 1; m.seed = 0;                                   // (the uniform and sampleOne's slot are not part of this record)
  *bytes = CSSM_FLEET_PMMH_LGCP_REC_BYTES(m.d);
  *fsub_count = 0;
  if (cap < *bytes) return fail(CSSM_EINVAL_ARG, "record of %zu bytes, room for %zu", *bytes, cap);
  std::vector<double> tab;
  const int prc = fleet_pmmh_lgcp_pack(m, t_prev, t, step, out, tab, 0);
  if (prc) return prc;
  *fsub_count = tab.size();
  if (tab.size() > fsub_cap || (!tab.empty() && !fsub_out)) return fail(CSSM_EINVAL_ARG, "sub-step table of %zu coefficients, room for %zu", tab.size(), fsub_cap);
  if (!tab.empty()) memcpy(fsub_out, tab.data(), tab.size() * 8u);
  return CSSM_OK;
}

static int fleet_ip_run(cssm_fleet* f, const uint64_t* off, const double* t, const double* y, const uint8_t* has_obs, double interval, bool pairing,
                        uint32_t n_traj, double* ll_out, const FleetIvOut& o, uint32_t* traj_out, int* rc_out) {
  const uint32_t S = f->S, n = f->n;
  const bool smooth = n_traj != 0u;
  const int d = f->d, rows = d + 1;
  int rc = CSSM_OK;
  for (uint32_t k = 0; k < S; ++k) {
    if ((rc = fleet_off_step("off", off, k))) return rc;
    if (off[k + 1] - off[k] > 0xfffffffeull) return fail(CSSM_EINVAL_ARG, "series %u: too many records", k);
  }
  HIP_TRY(hipSetDevice(f->device));
  rc = fleet_upload_par(f);
  if (rc) return rc;
  // chunks of series [cut[c], cut[c + 1]) whose history fits the cap; the buffers of the largest one
  const size_t RB = CSSM_FLEET_REC_BYTES(d), slice = (size_t)n * (8u * (size_t)d + 4u);
  std::vector<uint32_t> cut(1, 0u);
  size_t held = 0, need = 0, need_hist = 0, need_traj = 0;
  uint32_t widest = 0;
  for (uint32_t k = 0; k < S; ++k) {
    const size_t b = ((size_t)(off[k + 1] - off[k]) + 1u) * slice;
    if (k > cut.back() && held + b > f->ip_hist_max) { cut.push_back(k); held = 0; }
    held += b;
    if (held > need_hist) { need_hist = held; widest = cut.back(); }
  }
  cut.push_back(S);
  for (size_t c = 0; c + 1 < cut.size(); ++c) {
    need = std::max(need, fleet_ip_stage(f, off, cut[c], cut[c + 1]).bytes);
    need_traj = std::max(need_traj, ((size_t)(off[cut[c + 1]] - off[cut[c]]) + (cut[c + 1] - cut[c])) * (size_t)n_traj * 4u);
  }
  if (smooth && !f->d_bs_traj.reserve(need_traj, true)) return fail(CSSM_ENOMEM, "fleet smoothing: %zu bytes of trajectories", need_traj);
  if (!f->h_ip.reserve(need, true)) return fail(CSSM_ENOMEM, "fleet interpolation: %zu bytes of pinned staging", need);
  if (!f->d_ip.reserve(need, true)) return fail(CSSM_ENOMEM, "fleet interpolation: %zu bytes of records and results", need);
  if (!f->d_ip_hist.reserve(need_hist, false)) {
    if (need_hist > f->ip_hist_max)   // a series longer than the cap runs alone
      return fail(CSSM_ENOMEM, "fleet interpolation: series %u alone needs %zu bytes of lineage history ((T + 1) N (8 d + 4))", widest, need_hist);
    return fail(CSSM_ENOMEM, "fleet interpolation: %zu bytes of lineage history (CSSM_OPT_INTERP_CAP lowers it)", need_hist);
  }
  const FleetRanks r = fleet_ranks(smooth ? n_traj : n, interval);   // the ranks of as many values as a row summarises
  double ms[3] = {0.0, 0.0, 0.0};
  for (size_t c = 0; c + 1 < cut.size(); ++c) {
    const uint32_t k0 = cut[c], k1 = cut[c + 1], Sc = k1 - k0;
    const size_t R0 = (size_t)off[k0], Rc = (size_t)off[k1] - R0, Qc = Rc + Sc;
    const FleetIpStage st = fleet_ip_stage(f, off, k0, k1);
    unsigned long long* h_off = f->h_ip.at<unsigned long long>();
    unsigned char* h_recs = f->h_ip.at<unsigned char>(st.recs);
    double* h_fco = f->h_ip.at<double>(st.fco);
    const FleetSeries* h_ser = f->h_ip.at<const FleetSeries>(st.ser);
    const double* h_out = f->h_ip.at<const double>(st.out);
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
          StepRec rec;
          cssm_build_rec(&f->models[k], time, time, 0.0, 0, 0u, &rec);
          for (int cc = 0; cc < d; ++cc) fco[q * (size_t)d + cc] = rec.fco[cc];
        }
      }
    });
    if (Rc) {
      HIP_TRY(hipMemcpyAsync(f->d_ip.p, f->h_ip.p, st.ser, hipMemcpyHostToDevice, f->stream));
      HIP_TRY(hipEventRecord(f->ev_ip[0], f->stream));
      FleetLaunch l{};
      fleet_series_args(f, l);
      l.args.off = f->d_ip.at<const unsigned long long>(); l.args.recs = f->d_ip.at<const unsigned char>(st.recs);
      l.args.hist = f->d_ip_hist.at<double>(); l.args.hanc = f->d_ip_hist.at<uint32_t>(Qc * (size_t)d * n * 8u);
      l.args.hser = f->d_ip.at<FleetSeries>(st.ser); l.args.k0 = k0;
      l.n_series = Sc; l.kind = FleetKind::hist;
      rc = fleet_series_launch(d, l);
      if (rc) return rc;
      HIP_TRY(hipEventRecord(f->ev_ip[1], f->stream));
      if (smooth) {
        FleetBackLaunch bl;
        bl.args.n = n; bl.args.n_traj = n_traj;
        bl.args.hist = l.args.hist; bl.args.hanc = l.args.hanc;
        bl.args.off = l.args.off; bl.args.ser = l.args.hser; bl.args.recs = l.args.recs;
        bl.args.par = l.args.par; bl.args.k0 = k0;
        bl.args.traj = f->d_bs_traj.at<uint32_t>();
        bl.args.mk = f->base.mk;
        bl.d = d; bl.n_series = Sc; bl.stream = f->stream;
        bl.stage = f->bs_staging == 0 && (size_t)d * n * 8u <= CSSM_BACKSIM_STAGE_MAX;
        int hrc = cssm_fleet_backsim_launch(bl);
        if (hrc) return fail(CSSM_EHIP, "k_fleet_backsim: %s", hipGetErrorString((hipError_t)hrc));
        HIP_TRY(hipEventRecord(f->ev_ip[2], f->stream));
        FleetSmRowLaunch q;
        q.args.n = n; q.args.n_traj = n_traj; q.args.np2 = r.np2;
        q.args.hist = l.args.hist; q.args.traj = bl.args.traj;
        q.args.off = l.args.off; q.args.ser = l.args.hser;
        q.args.fco = f->d_ip.at<const double>(st.fco);
        q.args.out = f->d_ip.at<double>(st.out);
        q.args.mk = f->base.mk;
        q.args.lo_state = r.rk.lo_state; q.args.hi_state = r.rk.hi_state;
        q.args.lo_eta = r.rk.lo_eta; q.args.hi_eta = r.rk.hi_eta;
        q.d = d; q.n_series = Sc; q.stream = f->stream;
        hrc = cssm_fleet_smooth_rows_launch(q);
        if (hrc) return fail(CSSM_EHIP, "k_fleet_smooth_rows: %s", hipGetErrorString((hipError_t)hrc));
        HIP_TRY(hipEventRecord(f->ev_bs, f->stream));
        HIP_TRY(hipMemcpyAsync(f->h_ip.at<unsigned char>(st.ser), f->d_ip.at<unsigned char>(st.ser), st.bytes - st.ser, hipMemcpyDeviceToHost, f->stream));
        if (traj_out)   // the chunk's slices are the caller's rows off[k0] + k0 .. off[k1] + k1 - 1
          HIP_TRY(hipMemcpyAsync(traj_out + (R0 + k0) * (size_t)n_traj, bl.args.traj, Qc * (size_t)n_traj * 4u, hipMemcpyDeviceToHost, f->stream));
        HIP_TRY(hipStreamSynchronize(f->stream));
        float m0 = 0.f, m1 = 0.f, m2 = 0.f;
        if (hipEventElapsedTime(&m0, f->ev_ip[0], f->ev_ip[1]) == hipSuccess && hipEventElapsedTime(&m1, f->ev_ip[1], f->ev_ip[2]) == hipSuccess &&
            hipEventElapsedTime(&m2, f->ev_ip[2], f->ev_bs) == hipSuccess) {
          ms[0] += (double)m0; ms[1] += (double)m1; ms[2] += (double)m2;
        }
      } else {
        FleetLinLaunch q;
        q.args.n = n; q.args.np2 = r.np2; q.args.pairing = pairing ? 1u : 0u;
        q.args.hist = l.args.hist; q.args.hanc = l.args.hanc;
        q.args.off = l.args.off; q.args.ser = l.args.hser; q.args.recs = l.args.recs;
        q.args.fco = f->d_ip.at<const double>(st.fco);
        q.args.out = f->d_ip.at<double>(st.out);
        q.args.mk = f->base.mk;
        q.args.lo_state = r.rk.lo_state; q.args.hi_state = r.rk.hi_state;
        q.args.lo_eta = r.rk.lo_eta; q.args.hi_eta = r.rk.hi_eta;
        q.d = d; q.n_series = Sc; q.stream = f->stream;
        const int hrc = cssm_fleet_lineage_launch(q);
        if (hrc) return fail(CSSM_EHIP, "k_fleet_lineage: %s", hipGetErrorString((hipError_t)hrc));
        HIP_TRY(hipEventRecord(f->ev_ip[2], f->stream));
        HIP_TRY(hipMemcpyAsync(f->h_ip.at<unsigned char>(st.ser), f->d_ip.at<unsigned char>(st.ser), st.bytes - st.ser, hipMemcpyDeviceToHost, f->stream));
        HIP_TRY(hipStreamSynchronize(f->stream));
        float m0 = 0.f, m1 = 0.f;
        if (hipEventElapsedTime(&m0, f->ev_ip[0], f->ev_ip[1]) == hipSuccess && hipEventElapsedTime(&m1, f->ev_ip[1], f->ev_ip[2]) == hipSuccess) {
          ms[0] += (double)m0; ms[1] += (double)m1;
        }
      }
    }
    for (uint32_t kl = 0; kl < Sc; ++kl) {
      const uint32_t k = k0 + kl;
      const size_t a = (size_t)off[k], T = (size_t)off[k + 1] - a, lrow = a - R0 + kl, grow = a + k;
      if (T == 0) rc_out[k] = CSSM_EINVAL_ARG;                 // (the reference's minBy throws on an empty Vector)
      else rc_out[k] = h_ser[kl].err ? CSSM_ENONFINITE : CSSM_OK;
      const bool ok = rc_out[k] == CSSM_OK;
      ll_out[k] = ok ? h_ser[kl].ll : cssm_nan();
      for (size_t q = 0; q <= T; ++q)
        fleet_iv_row(f, k, h_out + (lrow + q) * (size_t)rows * 3u, h_fco + (lrow + q) * (size_t)d, ok, o, grow + q);
      if (traj_out && !ok) std::fill(traj_out + grow * (size_t)n_traj, traj_out + (grow + T + 1u) * (size_t)n_traj, 0xffffffffu);   // no trajectory
    }
  }
  if (smooth) { f->ms_bs[0] = ms[0]; f->ms_bs[1] = ms[1]; f->ms_bs[2] = ms[2]; f->bs_ran = true; }
  else { f->ms_ip[0] = ms[0]; f->ms_ip[1] = ms[1]; f->ip_ran = true; }
  return CSSM_OK;
}

extern "C" int cssm_fleet_interpolate_last_ms(cssm_fleet* f, double* ms2) {
  if (!f || !ms2) return fail(CSSM_EINVAL_ARG, "null argument");
  if (!f->ip_ran) return fail(CSSM_ESTATE, "no interpolation has run on this fleet (cssm_fleet_interpolate first)");
  ms2[0] = f->ms_ip[0]; ms2[1] = f->ms_ip[1];
  return CSSM_OK;
}

// ---- SimulateData.simPompModel of every series (model/Data.scala:64-73): cssm_simulate per series, in one launch per chunk of series.
// The fleet lends its device, stream, contract table, structure and the parameters of cssm_fleet_set_params; nothing it keeps per series
// is read or written on the device, so no series needs a cloud and none changes.
struct FleetSimStage {
  size_t keys, op, start, run, recs, bytes;
};
static FleetSimStage fleet_sim_stage(const cssm_fleet* f, size_t rows) {
  const size_t S = f->S;
  FleetSimStage st;
  st.keys = (S + 1u) * 8u;
  st.op = st.keys + S * 8u;
  st.start = st.op + fleet_pad8(S * sizeof(cssm_obs_params));
  st.run = st.start + S * sizeof(SimStart);
  st.recs = st.run + fleet_pad8(S * 4u);
  st.bytes = st.recs + rows * CSSM_FLEET_REC_BYTES(f->d);
  return st;
}

extern "C" int cssm_fleet_simulate(cssm_fleet* f, uint64_t n_paths, const double* t0, const uint64_t* off, const double* t, const uint64_t* keys,
                                   double* out, int* rc_out) {
  FLEET_LGCP_REFUSE(f, "cssm_fleet_simulate", FLEET_LGCP_SERVED);
  if (!f || !t0 || !off || !keys || !out || !rc_out) return fail(CSSM_EINVAL_ARG, "null argument");
  if (n_paths < 1 || n_paths > 0xffff0000ull) return fail(CSSM_EINVAL_ARG, "n_paths must be in [1, 2^32 - 2^16]");
  const uint32_t S = f->S;
  int rc = fleet_off_check(off, S);
  if (rc) return rc;
  if (off[S] && !t) return fail(CSSM_EINVAL_ARG, "null argument");
  const int d = f->d;
  const uint64_t n = n_paths, npairs = (n + 1) / 2;
  if (npairs * S > 0x7fffffffull * 64u) return fail(CSSM_EINVAL_ARG, "%u series x %llu paths are more than one launch serves", S, (unsigned long long)n);
  const size_t rows_all = (size_t)off[S] + S, row_doubles = (size_t)(d + 3) * n, row_bytes = row_doubles * 8u;
  // the series' own statuses, decided before the first device call
  std::vector<cssm_obs_params> ops(S);
  std::vector<uint32_t> run(S, 0u);
  std::string first_msg;
  size_t n_run = 0;
  for (uint32_t k = 0; k < S; ++k) {
    const size_t a = (size_t)off[k], b = (size_t)off[k + 1];
    rc_out[k] = CSSM_OK;
    memset(&ops[k], 0, sizeof(cssm_obs_params));
    int r = CSSM_OK;
    if (b - a >= 0xffffffffull) r = fail(CSSM_EINVAL_ARG, "too many times (the row at t0 draws its observation under step 2^32 - 1)");
    if (!r) r = cssm_obs_params_or_fail(f->base.obs_kind, f->obs_has_scale[k], f->obs_scale[k], f->base.obs_df, &ops[k]);
    if (!r && !std::isfinite(t0[k])) r = fail(CSSM_EINVAL_ARG, "t0 is not finite");
    if (!r) r = cssm_check_times(t + a, b - a, t0[k], "t0 =");
    if (r) {
      if (first_msg.empty()) first_msg = "series " + std::to_string(k) + ": " + cssm_last_error();
      rc_out[k] = r;
      continue;
    }
    run[k] = 1u;
    n_run += b - a + 1u;
  }
  if (n_run) {
    HIP_TRY(hipSetDevice(f->device));
    const size_t RB = CSSM_FLEET_REC_BYTES(d);
    const FleetSimStage st = fleet_sim_stage(f, rows_all);
    if (!f->h_sim.reserve(st.bytes, true)) return fail(CSSM_ENOMEM, "fleet simulate: %zu bytes of pinned staging", st.bytes);
    if (!f->d_sim.reserve(st.bytes, true)) return fail(CSSM_ENOMEM, "fleet simulate: %zu bytes of records", st.bytes);
    unsigned long long* h_off = f->h_sim.at<unsigned long long>();
    unsigned long long* h_keys = f->h_sim.at<unsigned long long>(st.keys);
    cssm_obs_params* h_op = f->h_sim.at<cssm_obs_params>(st.op);
    SimStart* h_start = f->h_sim.at<SimStart>(st.start);
    uint32_t* h_run = f->h_sim.at<uint32_t>(st.run);
    unsigned char* h_recs = f->h_sim.at<unsigned char>(st.recs);
    for (uint32_t k = 0; k <= S; ++k) h_off[k] = off[k];
    for (uint32_t k = 0; k < S; ++k) {
      const HostModel& m = f->models[k];
      h_keys[k] = keys[k]; h_op[k] = ops[k]; h_run[k] = run[k];
      for (int c = 0; c < CSSM_MAX_DIM; ++c) {
        h_start[k].m0[c] = c < d ? m.comp[c].m0 : 0.0;
        h_start[k].sd0[c] = c < d ? std::sqrt(m.comp[c].c0) : 0.0;
      }
    }
    fleet_parallel(S, n_run, [&](size_t lo, size_t hi) {
      for (size_t k = lo; k < hi; ++k) {
        if (!run[k]) continue;
        const size_t a = (size_t)off[k], b = (size_t)off[k + 1];
        unsigned char* r = h_recs + (a + k) * RB;
        fleet_pack_rec(f->models[k], t0[k], t0[k], 0.0, 0, CSSM_SIM_STEP_ROW0, r);
        double tp = t0[k];
        for (size_t s = a; s < b; ++s) {
          fleet_pack_rec(f->models[k], tp, t[s], 0.0, 0, (uint32_t)(s - a), r + (s - a + 1u) * RB);
          tp = t[s];
        }
      }
    });
    // chunks of series whose rows fit the cap (one series at least; a series beyond the cap runs alone, in windows of time indices)
    const size_t cap_rows = std::max<size_t>(1, f->fc_samp_max / row_bytes);
    std::vector<uint32_t> cut(1, 0u);
    for (uint32_t k = 0; k < S; ++k)
      if ((size_t)(off[k + 1] + k + 1u - (off[cut.back()] + cut.back())) > cap_rows && k > cut.back()) cut.push_back(k);
    cut.push_back(S);
    size_t most = 0;
    bool windows = false;
    for (size_t c = 0; c + 1 < cut.size(); ++c) {
      const size_t rws = (size_t)(off[cut[c + 1]] + cut[c + 1] - (off[cut[c]] + cut[c]));
      windows = windows || rws > cap_rows;
      most = std::max(most, std::min(rws, cap_rows));
    }
    if (!f->d_sim_out.reserve(most * row_bytes, false)) return fail(CSSM_ENOMEM, "fleet simulate: %zu bytes of rows", most * row_bytes);
    if (windows && !f->d_sim_carry.reserve((size_t)d * n * 8u, false)) return fail(CSSM_ENOMEM, "fleet simulate: %zu bytes of carried states", (size_t)d * n * 8u);
    CssmTemps tmp;
    hipEvent_t ev[2] = {nullptr, nullptr};
    for (hipEvent_t& e : ev) HIP_TRY(tmp.event(e));
    FleetSimArgs a;
    a.n = n;
    a.off = f->d_sim.at<const unsigned long long>();
    a.keys = f->d_sim.at<const unsigned long long>(st.keys);
    a.op = f->d_sim.at<const cssm_obs_params>(st.op);
    a.start = f->d_sim.at<const SimStart>(st.start);
    a.run = f->d_sim.at<const uint32_t>(st.run);
    a.recs = f->d_sim.at<const unsigned char>(st.recs);
    a.carry = f->d_sim_carry.at<double>();
    a.out = f->d_sim_out.at<double>();
    a.logtab = f->logtab.at<double>(); a.mk = f->base.mk;
    HIP_TRY(hipEventRecord(ev[0], f->stream));
    HIP_TRY(hipMemcpyAsync(f->d_sim.p, f->h_sim.p, st.bytes, hipMemcpyHostToDevice, f->stream));
    for (size_t c = 0; c + 1 < cut.size(); ++c) {
      const size_t ra = (size_t)(off[cut[c]] + cut[c]), rb = (size_t)(off[cut[c + 1]] + cut[c + 1]);
      a.k0 = cut[c]; a.n_series = cut[c + 1] - cut[c];
      // (a chunk beyond the cap is one series: its time indices in windows of cap_rows, the states carried between them)
      for (size_t w = 0; w < rb - ra; w += cap_rows) {
        const size_t wn = std::min(cap_rows, rb - ra - w);
        a.rb = (uint32_t)w; a.rn = (uint32_t)wn;
        a.from_carry = w > 0 ? 1 : 0; a.to_carry = w + wn < rb - ra ? 1 : 0;
        a.out_r0 = ra + w;
        const int hrc = cssm_fleet_simulate_launch(d, a, f->stream);
        if (hrc) return fail(CSSM_EHIP, "k_fleet_simulate: %s", hipGetErrorString((hipError_t)hrc));
        HIP_TRY(hipMemcpyAsync(out + (ra + w) * row_doubles, f->d_sim_out.p, wn * row_bytes, hipMemcpyDeviceToHost, f->stream));
        HIP_TRY(hipStreamSynchronize(f->stream));   // (the next launch writes the same buffer)
      }
    }
    HIP_TRY(hipEventRecord(ev[1], f->stream));
    HIP_TRY(hipStreamSynchronize(f->stream));
    if (hipEventElapsedTime(&f->ms_simulate, ev[0], ev[1]) != hipSuccess) f->ms_simulate = -1.f;
  }
  for (uint32_t k = 0; k < S; ++k)
    if (!run[k]) std::fill(out + (size_t)(off[k] + k) * row_doubles, out + (size_t)(off[k + 1] + k + 1u) * row_doubles, cssm_nan());
  if (!first_msg.empty()) (void)fail(CSSM_EINVAL_ARG, "%s", first_msg.c_str());   // (the call succeeds; the message names the first such series)
  return CSSM_OK;
}

extern "C" int cssm_fleet_simulate_last_ms(cssm_fleet* f, double* ms) {
  if (!f || !ms) return fail(CSSM_EINVAL_ARG, "null argument");
  if (f->ms_simulate < 0.f) return fail(CSSM_ESTATE, "no simulation has run on this fleet (cssm_fleet_simulate first)");
  *ms = (double)f->ms_simulate;
  return CSSM_OK;
}

extern "C" uint64_t cssm_fleet_observation_index(const cssm_fleet* f, uint32_t k) { return (f && k < f->S) ? f->step[k] : 0; }

extern "C" int cssm_fleet_get_particles(cssm_fleet* f, uint32_t k, double* out_dN) {
  if (!f || !out_dN) return fail(CSSM_EINVAL_ARG, "null argument");
  if (k >= f->S) return fail(CSSM_EINVAL_ARG, "series %u of %u", k, f->S);
  if (!f->live[k]) return fail(CSSM_ESTATE, "series %u has no cloud (not initialised, or its weights were unusable)", k);
  HIP_TRY(hipSetDevice(f->device));
  const uint32_t n = f->n;
  const double* src = f->state.at<double>() + ((size_t)k * 2u + (f->step[k] & 1u)) * f->d * n;
  hipLaunchKernelGGL(k_gather, dim3(grid_for(n, 256, 64)), dim3(256), 0, f->stream, src, (size_t)n, f->anc.at<uint32_t>() + (size_t)k * n, f->d_tmp.at<double>(), (size_t)n, (uint64_t)n,
                     f->d, (const double*)nullptr, (size_t)0, 0u);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(out_dN, f->d_tmp.p, (size_t)f->d * n * 8, hipMemcpyDeviceToHost, f->stream));
  HIP_TRY(hipStreamSynchronize(f->stream));
  return CSSM_OK;
}

extern "C" int cssm_fleet_get_ancestors(cssm_fleet* f, uint32_t k, uint32_t* out_N) {
  if (!f || !out_N) return fail(CSSM_EINVAL_ARG, "null argument");
  if (k >= f->S) return fail(CSSM_EINVAL_ARG, "series %u of %u", k, f->S);
  if (!f->live[k]) return fail(CSSM_ESTATE, "series %u has no cloud (not initialised, or its weights were unusable)", k);
  HIP_TRY(hipSetDevice(f->device));
  HIP_TRY(hipMemcpyAsync(out_N, f->anc.at<uint32_t>() + (size_t)k * f->n, (size_t)f->n * 4, hipMemcpyDeviceToHost, f->stream));
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

// The compact record of one event as an LGCP fleet uploads it, and the rows of the sub-step table it brings (fsub_off = 0: the table is
// this event's own).  No device.
extern "C" int cssm_fleet_pack_record_lgcp(const cssm_model_desc* desc, uint64_t n_particles, uint64_t seed, double t_prev, double t, uint32_t step,
                                           unsigned char* out, size_t cap, size_t* bytes, double* fsub_out, size_t fsub_cap, size_t* fsub_count) {
  if (!out || !bytes || !fsub_count) return fail(CSSM_EINVAL_ARG, "null argument");
  HostModel m;
  const int rc = cssm_build_model(&m, desc, false);
  if (rc) return rc;
  if (m.obs_kind != CSSM_OBS_LGCP) return fail(CSSM_EINVAL_DESC, "cssm_fleet_pack_record_lgcp packs LGCP events (obs_kind %d given): cssm_fleet_pack_record", m.obs_kind);
  m.n_global = n_particles; m.seed = seed;
  *bytes = CSSM_FLEET_LGCP_REC_BYTES(m.d);
  *fsub_count = 0;
  if (cap < *bytes) return fail(CSSM_EINVAL_ARG, "record of %zu bytes, room for %zu", *bytes, cap);
  std::vector<double> tab;
  const int prc = fleet_pack_rec_lgcp(m, t_prev, t, step, out, tab, 0);
  if (prc) return prc;
  *fsub_count = tab.size();
  if (tab.size() > fsub_cap || (!tab.empty() && !fsub_out)) return fail(CSSM_EINVAL_ARG, "sub-step table of %zu coefficients, room for %zu", tab.size(), fsub_cap);
  if (!tab.empty()) memcpy(fsub_out, tab.data(), tab.size() * 8u);
  return CSSM_OK;
}
