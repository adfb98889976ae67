// cssm_simulate_lgcp.hip -- event times of a log-Gaussian Cox process by thinning: SimulateData.simLGCP (model/Data.scala:110-149,
// simSdeStream :162-176) as cssm_simulate_lgcp.  See include/cssm_pf.h for the call, include/cssm_obs_draws.h for the counters and the
// two statements of the thinning (cssm_lgcp_candidate, cssm_lgcp_index), cssm_simulate_lgcp_plan.h for the host plan.
//
// Two kernels per chunk of paths.  k_lgcp_grid: one thread per PAIR of paths, as k_simulate (the transition streams are paired), the
// pair's states in registers over the whole grid, every transition under the one set of delta-coefficients (kernel arguments), the
// d + 3 rows of every grid index stored in k_simulate's layout and the running maximum of eta left per path.  k_lgcp_thin: one thread
// per path and one wave per block (many short loops of unequal length), the candidate loop of the contract, eta gathered from the grid
// rows; it runs twice under the same counters -- first to count a path's events, then, behind the exclusive scan of the counts (formed
// on the host, in path order), to write them.  Nothing but host memory outlives the call.
#include "cssm_internal.h"
#include "cssm_kernels.hip.h"
#include "cssm_posterior_move.hip.h"
#include "cssm_simulate.hip.h"
#include "cssm_simulate_lgcp_plan.h"

#include <algorithm>
#include <new>

#define CSSM_LGCP_THIN_BLOCK 64   /* one wave: a long loop holds up 63 neighbours at the most */

struct LgcpGridArgs {
  SimStart st;
  double coef[CSSM_MAX_DIM][4];   // the delta-coefficients: constant over the launch
  double delta;
  const double* fco;              // row g * fstride: the f coefficients of grid index g
  uint32_t fstride, n_grid;
  uint64_t i0, nc;                // the chunk: paths i0 .. i0 + nc - 1, i0 even
  uint64_t key;
  ModelK mk;
  const double* logtab;
  double* out;                    // [n_grid][d + 3][nc]
  double* ub;                     // [nc]
};

template <int D>
__global__ __launch_bounds__(CSSM_BLOCK) void k_lgcp_grid(const LgcpGridArgs a) {
  const double* tab = stage_log_table(a.logtab);
  const uint64_t p = (uint64_t)blockIdx.x * CSSM_BLOCK + threadIdx.x;
  if (p >= (a.nc + 1) / 2) return;   // (behind the table's barrier, the only one)
  const uint64_t la = 2 * p, ia = 2 * (a.i0 / 2 + p), nc = a.nc;   // (i0 is even; written so that the compiler sees an even ia, as k_simulate's 2 p)
  const bool hasb = la + 1 < nc;     // (a chunk is whole pairs but for the unpaired last path of an odd n_paths)
  const bool vec = hasb && (nc & 1u) == 0u;
  double xa[D], xb[D];
  sim_begin<D>(a.st, nullptr, 0, a.key, nc, ia, tab, xa);
  if (hasb) sim_begin<D>(a.st, nullptr, 0, a.key, nc, ia + 1, tab, xb);
  else {
#pragma unroll
    for (int k = 0; k < D; ++k) xb[k] = 0.0;
  }
  double ma = 0.0, mb = 0.0;
  for (uint32_t g = 0; g < a.n_grid; ++g) {
    if (g) {   // sim_rows' statements under step g - 1, dt = delta
      const uint32_t step = g - 1u;
      auto move = [&](int k, double& xk, double e) { transition_step(a.mk.kind(k), a.coef[k][0], a.coef[k][1], a.coef[k][2], a.coef[k][3], a.delta, xk, e); };
      if (hasb) {
        pair_normals_feed<D>(a.key, ia, step, tab, [&](int b, int k, double e) { move(k, b ? xb[k] : xa[k], e); });
      } else {
        double z[D];
        draw_normals<D>(a.key, ia, step, CSSM_STREAM_STEP, tab, z);
#pragma unroll
        for (int k = 0; k < D; ++k) move(k, xa[k], z[k]);
      }
    }
    const double* fco = a.fco + (size_t)g * a.fstride;
    const double ga = gamma_coef<D>(a.mk, fco, xa), ea = cssm_exp(ga);
    double gb = 0.0, eb = 0.0;
    if (hasb) { gb = gamma_coef<D>(a.mk, fco, xb); eb = cssm_exp(gb); }
    // the running maximum of the stored values; a NaN stays (NaN > x and x > NaN are both false)
    ma = (g == 0u || ea > ma || ea != ea) ? ea : ma;
    mb = (g == 0u || eb > mb || eb != eb) ? eb : mb;
    double* o = a.out + (size_t)g * (D + 3) * nc;
#pragma unroll
    for (int k = 0; k < D; ++k) sim_store(o + (size_t)k * nc, la, hasb, vec, xa[k], xb[k]);
    sim_store(o + (size_t)D * nc, la, hasb, vec, ga, gb);
    sim_store(o + (size_t)(D + 1) * nc, la, hasb, vec, ea, eb);
    sim_store(o + (size_t)(D + 2) * nc, la, hasb, vec, 0.0, 0.0);
  }
  a.ub[la] = ma;
  if (hasb) a.ub[la + 1] = mb;
}

struct LgcpThinArgs {
  uint64_t key, i0, nc;
  uint32_t n_grid, rows;          // rows = d + 3
  double start, end, delta;
  const double* grid_t;           // [n_grid]
  const double* grid;             // [n_grid][rows][nc]
  const double* ub;               // [nc]
  uint32_t* count;                // [nc] events     (written by the counting launch, read by the writing one)
  uint32_t* cand;                 // [nc] candidates taken
  int32_t* status;                // [nc] CSSM_LGCP_PATH_*
  const unsigned long long* off;  // [nc + 1] the exclusive scan of count, the chunk's first event = 0
  double* ev_t;                   // the chunk's events
  uint32_t* ev_idx;
  double* ev_rows;                // [events][rows]
};

template <bool WRITE>
__global__ __launch_bounds__(CSSM_LGCP_THIN_BLOCK) void k_lgcp_thin(const LgcpThinArgs a) {
  const uint64_t l = (uint64_t)blockIdx.x * CSSM_LGCP_THIN_BLOCK + threadIdx.x;
  if (l >= a.nc) return;
  const uint64_t i = a.i0 + l;
  const double ub = a.ub[l];
  int st = WRITE ? a.status[l] : cssm_lgcp_admit(ub, a.start, a.end);
  const uint32_t mine = WRITE ? a.count[l] : 0u;   // the events the counting launch found: nothing is written past them
  uint32_t c = 0u, e = 0u;
  if (st == CSSM_LGCP_PATH_OK) {
    double last = a.start;
    for (;;) {
      if (c == CSSM_LGCP_MAX_CANDIDATES) { st = CSSM_LGCP_PATH_TOO_MANY; break; }
      double E, V;
      cssm_lgcp_candidate(a.key, i, c, ub, &E, &V);
      const double t1 = last + E;
      if (!(t1 <= a.end)) break;
      c += 1u;
      const uint32_t k = cssm_lgcp_index(a.grid_t, a.n_grid, a.start, a.delta, t1);
      const double* col = a.grid + (size_t)k * a.rows * a.nc + l;
      if (V <= col[(size_t)(a.rows - 2u) * a.nc] / ub) {
        if (WRITE && e < mine) {
          const unsigned long long at = a.off[l] + e;
          a.ev_t[at] = t1;
          a.ev_idx[at] = k;
          double* r = a.ev_rows + (size_t)at * a.rows;
          for (uint32_t q = 0; q + 1u < a.rows; ++q) r[q] = col[(size_t)q * a.nc];
          r[a.rows - 1u] = 1.0;
        }
        e += 1u;
      }
      last = t1;
    }
  }
  if (!WRITE) {
    a.count[l] = st == CSSM_LGCP_PATH_OK ? e : 0u;
    a.cand[l] = c;
    a.status[l] = st;
  }
}

// ---- host

struct cssm_lgcp_sim {
  int d = 0;
  uint64_t n = 0, grid_points = 0, n_events = 0;
  bool keep_grid = false;
  std::vector<double> grid_t, grid, upper, ev_t, ev_rows;
  std::vector<uint64_t> ev_off;
  std::vector<uint32_t> cand, ev_idx;
  std::vector<int32_t> status;
};

static thread_local double g_lgcp_ms[2] = {-1.0, -1.0};   // the thread's last call: its grid kernels, its thinning launches

// the time between two events of the null stream, added to `ms`
static int lgcp_elapsed(hipEvent_t a, hipEvent_t b, double& ms) {
  float v = 0.f;
  HIP_TRY(hipEventSynchronize(b));
  HIP_TRY(hipEventElapsedTime(&v, a, b));
  ms += v;
  return CSSM_OK;
}

static int lgcp_run(const LgcpSimPlan& plan, uint64_t n, uint64_t key, double start, double end, size_t paths_per_launch, int device,
                    cssm_lgcp_sim& r) {
  int rc = cssm_use_device(device);
  if (rc) return rc;
  const int d = plan.m.d;
  const uint32_t rows = (uint32_t)(d + 3);
  const size_t G1 = plan.grid_t.size();
  const size_t pc = cssm_lgcp_paths_per_launch(d, n, G1, paths_per_launch, CSSM_LGCP_LAUNCH_CAP);
  r.d = d; r.n = n; r.grid_points = G1; r.n_events = 0;
  r.grid_t = plan.grid_t;
  r.upper.assign(n, 0.0); r.cand.assign(n, 0u); r.status.assign(n, 0); r.ev_off.assign(n + 1, 0u);
  if (r.keep_grid) r.grid.assign(G1 * rows * (size_t)n, 0.0);
  CssmTemps tmp;
  double *dgt = nullptr, *dfco = nullptr, *dtab = nullptr, *dgrid = nullptr, *dub = nullptr;
  uint32_t *dcount = nullptr, *dcand = nullptr;
  int32_t* dstatus = nullptr;
  unsigned long long* doff = nullptr;
  hipEvent_t ev[2] = {nullptr, nullptr};
  HIP_ALLOC(tmp, dgt, G1 * 8u);
  HIP_ALLOC(tmp, dfco, plan.fco.size() * 8u);
  HIP_ALLOC(tmp, dtab, sizeof(CSSM_TAB));
  HIP_ALLOC(tmp, dgrid, G1 * rows * pc * 8u);
  HIP_ALLOC(tmp, dub, pc * 8u);
  HIP_ALLOC(tmp, dcount, pc * 4u);
  HIP_ALLOC(tmp, dcand, pc * 4u);
  HIP_ALLOC(tmp, dstatus, pc * 4u);
  HIP_ALLOC(tmp, doff, (pc + 1) * 8u);
  for (hipEvent_t& e : ev) HIP_TRY(tmp.event(e));
  HIP_TRY(hipMemcpy(dgt, plan.grid_t.data(), G1 * 8u, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(dfco, plan.fco.data(), plan.fco.size() * 8u, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(dtab, CSSM_TAB, sizeof(CSSM_TAB), hipMemcpyHostToDevice));
  LgcpGridArgs ga;
  memcpy(ga.st.m0, plan.m0, sizeof ga.st.m0); memcpy(ga.st.sd0, plan.sd0, sizeof ga.st.sd0);
  memcpy(ga.coef, plan.coef, sizeof ga.coef);
  ga.delta = plan.delta; ga.fco = dfco; ga.fstride = (uint32_t)plan.fstride; ga.n_grid = (uint32_t)G1;
  ga.key = key; ga.mk = plan.m.mk; ga.logtab = dtab; ga.out = dgrid; ga.ub = dub;
  LgcpThinArgs ta;
  ta.key = key; ta.n_grid = (uint32_t)G1; ta.rows = rows; ta.start = start; ta.end = end; ta.delta = plan.delta;
  ta.grid_t = dgt; ta.grid = dgrid; ta.ub = dub; ta.count = dcount; ta.cand = dcand; ta.status = dstatus; ta.off = doff;
  std::vector<uint32_t> count(pc);
  std::vector<unsigned long long> off(pc + 1);
  double ms[2] = {0.0, 0.0};
  for (uint64_t i0 = 0; i0 < n; i0 += pc) {
    const uint64_t nc = std::min<uint64_t>(pc, n - i0);
    const unsigned gblocks = (unsigned)(((nc + 1) / 2 + CSSM_BLOCK - 1) / CSSM_BLOCK);
    const unsigned tblocks = (unsigned)((nc + CSSM_LGCP_THIN_BLOCK - 1) / CSSM_LGCP_THIN_BLOCK);
    ga.i0 = i0; ga.nc = nc;
    HIP_TRY(hipEventRecord(ev[0], 0));
    DISPATCH_D(d, hipLaunchKernelGGL(k_lgcp_grid<D>, dim3(gblocks), dim3(CSSM_BLOCK), 0, 0, ga));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(ev[1], 0));
    rc = lgcp_elapsed(ev[0], ev[1], ms[0]);
    if (rc) return rc;
    // the counting launch
    ta.i0 = i0; ta.nc = nc; ta.ev_t = nullptr; ta.ev_idx = nullptr; ta.ev_rows = nullptr;
    HIP_TRY(hipEventRecord(ev[0], 0));
    hipLaunchKernelGGL(k_lgcp_thin<false>, dim3(tblocks), dim3(CSSM_LGCP_THIN_BLOCK), 0, 0, ta);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(ev[1], 0));
    rc = lgcp_elapsed(ev[0], ev[1], ms[1]);
    if (rc) return rc;
    HIP_TRY(hipMemcpy(count.data(), dcount, nc * 4u, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(r.cand.data() + i0, dcand, nc * 4u, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(r.status.data() + i0, dstatus, nc * 4u, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(r.upper.data() + i0, dub, nc * 8u, hipMemcpyDeviceToHost));
    if (r.keep_grid)
      HIP_TRY(hipMemcpy2D(r.grid.data() + i0, (size_t)n * 8u, dgrid, (size_t)nc * 8u, (size_t)nc * 8u, G1 * rows, hipMemcpyDeviceToHost));
    // the exclusive scan of the counts, in path order
    off[0] = 0;
    for (uint64_t l = 0; l < nc; ++l) {
      off[l + 1] = off[l] + count[l];
      r.ev_off[i0 + l + 1] = r.ev_off[i0] + off[l + 1];
    }
    const size_t ne = (size_t)off[nc], e0 = (size_t)r.ev_off[i0];
    if (ne == 0) continue;
    r.ev_t.resize(e0 + ne); r.ev_idx.resize(e0 + ne); r.ev_rows.resize((e0 + ne) * rows);
    CssmTemps evtmp;   // the chunk's events: released before the next chunk asks for its own
    HIP_ALLOC(evtmp, ta.ev_t, ne * 8u);
    HIP_ALLOC(evtmp, ta.ev_idx, ne * 4u);
    HIP_ALLOC(evtmp, ta.ev_rows, ne * rows * 8u);
    HIP_TRY(hipMemcpy(doff, off.data(), (nc + 1) * 8u, hipMemcpyHostToDevice));
    HIP_TRY(hipEventRecord(ev[0], 0));
    hipLaunchKernelGGL(k_lgcp_thin<true>, dim3(tblocks), dim3(CSSM_LGCP_THIN_BLOCK), 0, 0, ta);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(ev[1], 0));
    rc = lgcp_elapsed(ev[0], ev[1], ms[1]);
    if (rc) return rc;
    HIP_TRY(hipMemcpy(r.ev_t.data() + e0, ta.ev_t, ne * 8u, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(r.ev_idx.data() + e0, ta.ev_idx, ne * 4u, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(r.ev_rows.data() + e0 * rows, ta.ev_rows, ne * rows * 8u, hipMemcpyDeviceToHost));
  }
  r.n_events = r.ev_off[n];
  g_lgcp_ms[0] = ms[0]; g_lgcp_ms[1] = ms[1];
  return CSSM_OK;
}

extern "C" int cssm_simulate_lgcp(const cssm_model_desc* desc, uint64_t n_paths, uint64_t key, double start, double end, int precision, int flags,
                                  size_t paths_per_launch, int device, cssm_lgcp_sim** out) {
  LgcpSimPlan plan;
  int rc = cssm_simulate_lgcp_plan(desc, n_paths, start, end, precision, out, &plan);
  if (rc) return rc;
  if (flags & ~CSSM_LGCP_SIM_KEEP_GRID) return fail(CSSM_EINVAL_ARG, "unknown flags 0x%x", (unsigned)flags);
  cssm_lgcp_sim* r = new (std::nothrow) cssm_lgcp_sim;
  if (!r) return fail(CSSM_ENOMEM, "out of host memory");
  r->keep_grid = (flags & CSSM_LGCP_SIM_KEEP_GRID) != 0;
  try {
    rc = lgcp_run(plan, n_paths, key, start, end, paths_per_launch, device, *r);
  } catch (const std::bad_alloc&) {
    rc = fail(CSSM_ENOMEM, "out of host memory for the result (%zu grid points x %d rows x %llu paths)", plan.grid_t.size(), plan.m.d + 3,
              (unsigned long long)n_paths);
  }
  if (rc) { delete r; return rc; }
  *out = r;
  return CSSM_OK;
}

extern "C" int cssm_lgcp_sim_shape(const cssm_lgcp_sim* s, int* d, uint64_t* n_paths, uint64_t* grid_points, uint64_t* n_events) {
  if (!s) return fail(CSSM_EINVAL_ARG, "null argument");
  if (d) *d = s->d;
  if (n_paths) *n_paths = s->n;
  if (grid_points) *grid_points = s->grid_points;
  if (n_events) *n_events = s->n_events;
  return CSSM_OK;
}

template <class T>
static void lgcp_copy(const std::vector<T>& v, T* to) {
  if (to && !v.empty()) memcpy(to, v.data(), v.size() * sizeof(T));
}

extern "C" int cssm_lgcp_sim_grid_times(const cssm_lgcp_sim* s, double* t) {
  if (!s) return fail(CSSM_EINVAL_ARG, "null argument");
  lgcp_copy(s->grid_t, t);
  return CSSM_OK;
}

extern "C" int cssm_lgcp_sim_grid(const cssm_lgcp_sim* s, double* rows) {
  if (!s) return fail(CSSM_EINVAL_ARG, "null argument");
  if (!s->keep_grid) return fail(CSSM_ESTATE, "the grid rows were not kept (CSSM_LGCP_SIM_KEEP_GRID)");
  lgcp_copy(s->grid, rows);
  return CSSM_OK;
}

extern "C" int cssm_lgcp_sim_paths(const cssm_lgcp_sim* s, uint64_t* ev_off, double* upper, uint32_t* candidates, int32_t* status) {
  if (!s) return fail(CSSM_EINVAL_ARG, "null argument");
  lgcp_copy(s->ev_off, ev_off); lgcp_copy(s->upper, upper); lgcp_copy(s->cand, candidates); lgcp_copy(s->status, status);
  return CSSM_OK;
}

extern "C" int cssm_lgcp_sim_events(const cssm_lgcp_sim* s, double* ev_t, uint32_t* ev_idx, double* ev_rows) {
  if (!s) return fail(CSSM_EINVAL_ARG, "null argument");
  lgcp_copy(s->ev_t, ev_t); lgcp_copy(s->ev_idx, ev_idx); lgcp_copy(s->ev_rows, ev_rows);
  return CSSM_OK;
}

extern "C" void cssm_lgcp_sim_destroy(cssm_lgcp_sim* s) { delete s; }

extern "C" int cssm_simulate_lgcp_last_ms(double* ms2) {
  if (!ms2) return fail(CSSM_EINVAL_ARG, "null argument");
  if (g_lgcp_ms[0] < 0.0) return fail(CSSM_ESTATE, "no Cox-process simulation has run on this thread");
  ms2[0] = g_lgcp_ms[0]; ms2[1] = g_lgcp_ms[1];
  return CSSM_OK;
}
