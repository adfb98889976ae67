// cssm_simulate.hip -- series drawn from the model itself: SimulateData.simPompModel (model/Data.scala:64-73, simStep :186-193), for one
// model (cssm_simulate, cssm_simulate_from: k_simulate) and for every series of a fleet in one launch per chunk (cssm_fleet_simulate,
// whose host side is cssm_fleet.hip: k_fleet_simulate).  See include/cssm_pf.h for the contract, include/cssm_obs_draws.h for the counters.
//
// One thread owns one PAIR of paths (the transition streams are paired: every Philox block serves both) and loops over the launch's
// records with the pair's states in registers: the transition (CSSM_STREAM_STEP), gamma and eta at the record's time, one observation
// draw (CSSM_STREAM_OBS), and the d + 3 output rows of the time index -- the only stores, along the paths.  No order keys, no partial
// sums, no barrier behind the staging of the contract's table, no LDS beyond that table.  The chain of a pair is what forecast_body runs
// per horizon, through the same device functions: pair_normals_feed / draw_normals, transition_step, gamma_coef, link_of,
// cssm_obs_draw_one -- so a handle's forecast samples and these rows are equal bits.  Both kernels run sim_rows, written once; they
// differ in where a thread finds its records (the launch's StepRec array | its series' compact records) and its model's constants.
#include "cssm_internal.h"
#include "cssm_kernels.hip.h"
#include "cssm_posterior_move.hip.h"
#include "cssm_fleet.hip.h"
#include "cssm_simulate.hip.h"
#include "cssm_simulate_plan.h"

#include <algorithm>

#define CSSM_SIM_FLEET_BLOCK 64   /* one wave: a fleet of few paths per series spreads over the compute units */

// what a time index needs of its record: the increment, the 4 transition coefficients per component, the f coefficients
struct SimRec {
  double dt;
  const double* __restrict__ coef;
  const double* __restrict__ fco;
};

// Time indices g0 .. g0 + hc - 1 of one pair.  `row0`: time index 0 is the row at t0 (no transition, CSSM_SIM_STEP_ROW0); every other
// time index g moves and draws under step step_base + g - row0.  rec(j) = the record of time index g0 + j.
template <int D, class RecAt>
__device__ __forceinline__ void sim_rows(const ModelK& mk, const cssm_obs_params& op, uint64_t key, uint64_t n, uint64_t ia, bool hasb, uint32_t g0,
                                         uint32_t hc, uint32_t row0, uint32_t step_base, const double* tab, RecAt&& rec, double (&xa)[D],
                                         double (&xb)[D], double* __restrict__ out) {
  const bool vec = hasb && (n & 1u) == 0u;
  for (uint32_t j = 0; j < hc; ++j) {
    const SimRec r = rec(j);
    const uint32_t g = g0 + j;
    const bool first = row0 != 0u && g == 0u;
    const uint32_t step = first ? CSSM_SIM_STEP_ROW0 : step_base + g - row0;
    if (!first) {
      auto move = [&](int k, double& xk, double e) { transition_step(mk.kind(k), r.coef[4 * k], r.coef[4 * k + 1], r.coef[4 * k + 2], r.coef[4 * k + 3], r.dt, xk, e); };
      if (hasb) {
        pair_normals_feed<D>(key, ia, step, tab, [&](int b, int k, double e) { move(k, b ? xb[k] : xa[k], e); });
      } else {   // the unpaired last path of an odd count: propagate_one's statements (draw_normals, then every component)
        double z[D];
        draw_normals<D>(key, ia, step, CSSM_STREAM_STEP, tab, z);
#pragma unroll
        for (int k = 0; k < D; ++k) move(k, xa[k], z[k]);
      }
    }
    const double ga = gamma_coef<D>(mk, r.fco, xa);
    const double ea = link_of(mk.obs_kind, ga);
    cssm_obs_stream sa = cssm_obs_stream_at(key, ia, step);
    const double oa = cssm_obs_draw_one(&op, ea, &sa, tab);
    double gb = 0.0, eb = 0.0, ob = 0.0;
    if (hasb) {
      gb = gamma_coef<D>(mk, r.fco, xb);
      eb = link_of(mk.obs_kind, gb);
      cssm_obs_stream sb = cssm_obs_stream_at(key, ia + 1, step);
      ob = cssm_obs_draw_one(&op, eb, &sb, tab);
    }
    double* o = out + (size_t)j * (D + 3) * n;
#pragma unroll
    for (int k = 0; k < D; ++k) sim_store(o + (size_t)k * n, ia, hasb, vec, xa[k], xb[k]);
    sim_store(o + (size_t)D * n, ia, hasb, vec, ga, gb);
    sim_store(o + (size_t)(D + 1) * n, ia, hasb, vec, ea, eb);
    sim_store(o + (size_t)(D + 2) * n, ia, hasb, vec, oa, ob);
  }
}

// where a pair leaves its states for the next launch (sim_begin, which picks them up, and sim_store: cssm_simulate.hip.h)
template <int D>
__device__ __forceinline__ void sim_end(double* __restrict__ carry, uint64_t n, uint64_t ia, bool hasb, const double (&xa)[D], const double (&xb)[D]) {
#pragma unroll
  for (int k = 0; k < D; ++k) {
    carry[(size_t)k * n + ia] = xa[k];
    if (hasb) carry[(size_t)k * n + ia + 1] = xb[k];
  }
}

// ---- one model: grid = the pairs of paths, CSSM_BLOCK threads per block
template <int D>
__global__ __launch_bounds__(CSSM_BLOCK) void k_simulate(SimStart st, double* __restrict__ carry, int from_carry, int to_carry, uint64_t n,
                                                         const StepRec* __restrict__ recs, uint32_t g0, uint32_t hc, uint32_t row0, uint32_t step_base,
                                                         ModelK mk, uint64_t key, cssm_obs_params op, const double* __restrict__ logtab,
                                                         double* __restrict__ out) {
  const double* tab = stage_log_table(logtab);
  const uint64_t p = (uint64_t)blockIdx.x * CSSM_BLOCK + threadIdx.x;
  if (p >= (n + 1) / 2) return;   // (behind the table's barrier, the only one)
  const uint64_t ia = 2 * p;
  const bool hasb = ia + 1 < n;
  double xa[D], xb[D];
  sim_begin<D>(st, carry, from_carry, key, n, ia, tab, xa);
  if (hasb) sim_begin<D>(st, carry, from_carry, key, n, ia + 1, tab, xb);
  else {
#pragma unroll
    for (int k = 0; k < D; ++k) xb[k] = 0.0;
  }
  sim_rows<D>(mk, op, key, n, ia, hasb, g0, hc, row0, step_base, tab,
              [&](uint32_t j) { const StepRec* r = recs + g0 + j; return SimRec{r->dt, &r->coef[0][0], r->fco}; }, xa, xb, out);
  if (to_carry) sim_end<D>(carry, n, ia, hasb, xa, xb);
}

// ---- a fleet: thread p = pair p % npairs of series k0 + p / npairs; consecutive threads take consecutive pairs of one series, then the
// next series, so a fleet of single paths fills its waves.  A thread reads its series' key, constants and compact records itself.
template <int D>
__global__ __launch_bounds__(CSSM_SIM_FLEET_BLOCK) void k_fleet_simulate(const FleetSimArgs a) {
  const double* tab = stage_log_table(a.logtab);
  const uint64_t n = a.n, npairs = (n + 1) / 2;
  const uint64_t p = (uint64_t)blockIdx.x * CSSM_SIM_FLEET_BLOCK + threadIdx.x;
  if (p >= npairs * a.n_series) return;
  const uint32_t ks = (uint32_t)(p / npairs), k = a.k0 + ks;
  if (!a.run[k]) return;
  const unsigned long long r0 = a.off[k] + k, rows = a.off[k + 1] - a.off[k] + 1u;   // the series' first row, its time indices
  if ((unsigned long long)a.rb >= rows) return;
  const uint32_t hc = (rows - a.rb < (unsigned long long)a.rn) ? (uint32_t)(rows - a.rb) : a.rn;
  const uint64_t ia = 2 * (p % npairs);
  const bool hasb = ia + 1 < n;
  const uint64_t key = a.keys[k];
  const cssm_obs_params op = a.op[k];
  double* carry = a.carry + (size_t)ks * D * n;
  double xa[D], xb[D];
  sim_begin<D>(a.start[k], carry, a.from_carry, key, n, ia, tab, xa);
  if (hasb) sim_begin<D>(a.start[k], carry, a.from_carry, key, n, ia + 1, tab, xb);
  else {
#pragma unroll
    for (int q = 0; q < D; ++q) xb[q] = 0.0;
  }
  const size_t RB = CSSM_FLEET_REC_BYTES(D);
  const unsigned char* recs = a.recs + (size_t)(r0 + a.rb) * RB;
  sim_rows<D>(a.mk, op, key, n, ia, hasb, a.rb, hc, 1u, 0u, tab,
              [&](uint32_t j) {
                const unsigned char* r = recs + (size_t)j * RB;
                const double* tail = reinterpret_cast<const double*>(r + sizeof(FleetRecHead));
                return SimRec{reinterpret_cast<const FleetRecHead*>(r)->dt, tail, tail + 4 * D};
              },
              xa, xb, a.out + (size_t)(r0 + a.rb - a.out_r0) * (D + 3) * n);
  if (a.to_carry) sim_end<D>(carry, n, ia, hasb, xa, xb);
}

int cssm_fleet_simulate_launch(int d, const FleetSimArgs& a, hipStream_t stream) {
  const uint64_t threads = ((a.n + 1) / 2) * a.n_series;
  const unsigned blocks = (unsigned)((threads + CSSM_SIM_FLEET_BLOCK - 1) / CSSM_SIM_FLEET_BLOCK);
  DISPATCH_D(d, hipLaunchKernelGGL(k_fleet_simulate<D>, dim3(blocks), dim3(CSSM_SIM_FLEET_BLOCK), 0, stream, a));
  return (int)hipGetLastError();
}

// ---- host: one model

static thread_local double g_sim_ms = -1.0;   // device time of the thread's last cssm_simulate / cssm_simulate_from (its kernels, HIP events)

// run a plan: the chunks of time indices, the states carried on the device between them
static int simulate_run(const SimPlan& plan, uint64_t n, uint64_t key, const double* x, uint32_t step_base, size_t rows_per_launch, int device,
                        double* out) {
  const size_t rows = plan.recs.size();
  if (rows == 0) return CSSM_OK;
  int rc = cssm_use_device(device);
  if (rc) return rc;
  const int d = plan.m.d;
  const size_t row_bytes = (size_t)(d + 3) * n * 8u;
  const size_t hc = cssm_simulate_rows_per_launch(d, n, rows, rows_per_launch, (size_t)1 << 30);
  const bool chunked = hc < rows;
  const uint32_t row0 = x ? 0u : 1u;
  const unsigned blocks = (unsigned)(((n + 1) / 2 + CSSM_BLOCK - 1) / CSSM_BLOCK);
  SimStart st;
  memcpy(st.m0, plan.m0, sizeof st.m0); memcpy(st.sd0, plan.sd0, sizeof st.sd0);
  CssmTemps tmp;
  StepRec* drec = nullptr; double *carry = nullptr, *dout = nullptr, *dtab = nullptr;
  hipEvent_t ev[2] = {nullptr, nullptr};
  HIP_ALLOC(tmp, drec, rows * sizeof(StepRec));
  HIP_ALLOC(tmp, dout, hc * row_bytes);
  HIP_ALLOC(tmp, dtab, sizeof(CSSM_TAB));
  if (chunked || x) HIP_ALLOC(tmp, carry, (size_t)d * n * 8u);
  for (hipEvent_t& e : ev) HIP_TRY(tmp.event(e));
  HIP_TRY(hipMemcpy(drec, plan.recs.data(), rows * sizeof(StepRec), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(dtab, CSSM_TAB, sizeof(CSSM_TAB), hipMemcpyHostToDevice));
  if (x) HIP_TRY(hipMemcpy(carry, x, (size_t)d * n * 8u, hipMemcpyHostToDevice));
  double ms = 0.0;
  for (size_t g0 = 0; g0 < rows; g0 += hc) {
    const size_t hn = std::min(hc, rows - g0);
    const int from_carry = (x || g0 > 0) ? 1 : 0, to_carry = (chunked && g0 + hn < rows) ? 1 : 0;
    HIP_TRY(hipEventRecord(ev[0], 0));
    DISPATCH_D(d, hipLaunchKernelGGL(k_simulate<D>, dim3(blocks), dim3(CSSM_BLOCK), 0, 0, st, carry, from_carry, to_carry, n, (const StepRec*)drec,
                                     (uint32_t)g0, (uint32_t)hn, row0, step_base, plan.m.mk, key, plan.op, (const double*)dtab, dout));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(ev[1], 0));
    HIP_TRY(hipMemcpy(out + g0 * (size_t)(d + 3) * n, dout, hn * row_bytes, hipMemcpyDeviceToHost));
    float a = 0.f;
    HIP_TRY(hipEventElapsedTime(&a, ev[0], ev[1]));
    ms += a;
  }
  g_sim_ms = ms;
  return CSSM_OK;
}

extern "C" int cssm_simulate(const cssm_model_desc* desc, uint64_t n_paths, uint64_t key, double t0, const double* t, size_t T, size_t rows_per_launch,
                             int device, double* out) {
  SimPlan plan;
  const int rc = cssm_simulate_plan(desc, n_paths, key, nullptr, 0u, t0, t, T, out, &plan);
  if (rc) return rc;
  return simulate_run(plan, n_paths, key, nullptr, 0u, rows_per_launch, device, out);
}

extern "C" int cssm_simulate_from(const cssm_model_desc* desc, uint64_t n_paths, uint64_t key, const double* x, uint32_t first_step, double t0,
                                  const double* t, size_t T, size_t rows_per_launch, int device, double* out) {
  if (!x) return fail(CSSM_EINVAL_ARG, "null argument");
  SimPlan plan;
  const int rc = cssm_simulate_plan(desc, n_paths, key, x, first_step, t0, t, T, out, &plan);
  if (rc) return rc;
  return simulate_run(plan, n_paths, key, x, first_step, rows_per_launch, device, out);
}

extern "C" int cssm_simulate_last_ms(double* ms) {
  if (!ms) return fail(CSSM_EINVAL_ARG, "null argument");
  if (g_sim_ms < 0.0) return fail(CSSM_ESTATE, "no simulation has run on this thread");
  *ms = g_sim_ms;
  return CSSM_OK;
}
