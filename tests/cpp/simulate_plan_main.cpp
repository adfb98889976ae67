// Stand-alone driver of the host side of SimulateData (csrc/cssm_simulate_plan.cpp over csrc/cssm_model.cpp): every refusal that is decided
// before the first device call and the records of accepted calls, for a build under -fsanitize=address,undefined
// (tests/test_simulate_host.py compiles and runs it).  No HIP, no device.  Exit status 0 = every expectation held.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "cssm_simulate_plan.h"

extern "C" const char* cssm_last_error(void);
// cssm_model.cpp's PMMH loop drives a filter handle through the C ABI; nothing here reaches it, the linker wants the names
extern "C" int32_t cssm_pf_dim(const cssm_pf*) { return 0; }
extern "C" int cssm_pf_reseed(cssm_pf*, uint64_t) { return CSSM_ESTATE; }
extern "C" int cssm_pf_set_params(cssm_pf*, const cssm_model_desc*) { return CSSM_ESTATE; }
extern "C" int cssm_pf_filter(cssm_pf*, const double*, const double*, const uint8_t*, size_t, double*, double*, int32_t*, double*) { return CSSM_ESTATE; }

static int failures = 0;
#define EXPECT(cond)                                                          \
  do {                                                                        \
    if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } \
  } while (0)

struct Leaf {
  std::vector<double> m0, c0, mu, phi, sigma;
  cssm_leaf_desc d;
};

static void ou_leaf(Leaf& l, int dim, int f_kind, int period, int harmonics, int has_scale, double scale) {
  l.m0.assign(1, 0.1); l.c0.assign(1, 0.0); l.mu.assign(1, 0.5); l.phi.assign(1, 0.55); l.sigma.assign(1, -1.2);
  std::memset(&l.d, 0, sizeof l.d);
  l.d.sde_kind = CSSM_SDE_OU; l.d.dim = dim; l.d.f_kind = f_kind; l.d.period = period; l.d.harmonics = harmonics;
  l.d.has_scale = has_scale; l.d.scale = scale;
  l.d.m0 = l.m0.data(); l.d.n_m0 = 1; l.d.c0 = l.c0.data(); l.d.n_c0 = 1; l.d.mu = l.mu.data(); l.d.n_mu = 1;
  l.d.phi = l.phi.data(); l.d.n_phi = 1; l.d.sigma = l.sigma.data(); l.d.n_sigma = 1;
}

static bool says(const char* word) { return std::strstr(cssm_last_error(), word) != nullptr; }

int main() {
  Leaf a, b;
  ou_leaf(a, 1, CSSM_F_FIRST, 0, 0, 1, -1.0);
  ou_leaf(b, 2, CSSM_F_SEASONAL, 24, 1, 0, 0.0);
  cssm_leaf_desc leaves[2] = {a.d, b.d};
  cssm_model_desc desc;
  std::memset(&desc, 0, sizeof desc);
  desc.n_leaves = 2; desc.obs_kind = CSSM_OBS_POISSON; desc.leaves = leaves;
  const double t[5] = {0.5, 0.5, 1.75, 3.0, 7.25};
  double out[1] = {0.0};
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();

  {  // an accepted call: T + 1 records, the first one the row at t0
    SimPlan p;
    EXPECT(cssm_simulate_plan(&desc, 5, 42, nullptr, 0u, 0.0, t, 5, out, &p) == CSSM_OK);
    EXPECT(p.recs.size() == 6 && p.m.d == 3 && p.m.n_global == 5 && p.m.seed == 42);
    EXPECT(p.recs[0].dt == 0.0 && p.recs[0].step == CSSM_SIM_STEP_ROW0 && p.recs[0].has_obs == 0);
    EXPECT(p.recs[1].dt == 0.5 && p.recs[1].step == 0u && p.recs[2].dt == 0.0 && p.recs[5].dt == 4.25 && p.recs[5].step == 4u);
    EXPECT(p.recs[0].fco[0] == 1.0 && p.recs[0].fco[1] == 1.0 && p.recs[0].fco[2] == 0.0);   // F at t0 = 0: (1, cos 0, sin 0)
    EXPECT(p.m0[0] == 0.1 && p.sd0[0] == 1.0 && p.m0[3] == 0.0 && p.sd0[15] == 0.0 && p.op.kind == CSSM_OBS_POISSON);
    SimPlan q;   // T = 0 with no times: the row at t0 alone
    EXPECT(cssm_simulate_plan(&desc, 1, 42, nullptr, 0u, 2.0, nullptr, 0, out, &q) == CSSM_OK && q.recs.size() == 1);
  }
  {  // a continued call: T records, steps first_step ..
    SimPlan p;
    const double x[6] = {0, 1, 2, 3, 4, 5};
    EXPECT(cssm_simulate_plan(&desc, 2, 42, x, 7u, 0.25, t, 5, out, &p) == CSSM_OK);
    EXPECT(p.recs.size() == 5 && p.recs[0].step == 7u && p.recs[0].dt == 0.25 && p.recs[4].step == 11u);
    double bad[6] = {0, 1, 2, inf, 4, 5};
    EXPECT(cssm_simulate_plan(&desc, 2, 42, bad, 7u, 0.25, t, 5, out, &p) == CSSM_EINVAL_ARG && says("component 1 of path 1"));
    EXPECT(cssm_simulate_plan(&desc, 2, 42, x, 0xFFFFFFFBu, 0.25, t, 5, out, &p) == CSSM_EINVAL_ARG && says("first_step + T"));
    EXPECT(cssm_simulate_plan(&desc, 2, 42, x, 0xFFFFFFFAu, 0.25, t, 5, out, &p) == CSSM_OK && p.recs[4].step == 0xFFFFFFFEu);
  }
  {  // the refusals
    SimPlan p;
    EXPECT(cssm_simulate_plan(nullptr, 5, 42, nullptr, 0u, 0.0, t, 5, out, &p) == CSSM_EINVAL_ARG && says("null argument"));
    EXPECT(cssm_simulate_plan(&desc, 5, 42, nullptr, 0u, 0.0, t, 5, nullptr, &p) == CSSM_EINVAL_ARG && says("null argument"));
    EXPECT(cssm_simulate_plan(&desc, 5, 42, nullptr, 0u, 0.0, nullptr, 5, out, &p) == CSSM_EINVAL_ARG && says("null argument"));
    EXPECT(cssm_simulate_plan(&desc, 0, 42, nullptr, 0u, 0.0, t, 5, out, &p) == CSSM_EINVAL_ARG && says("n_paths"));
    EXPECT(cssm_simulate_plan(&desc, 5, 42, nullptr, 0u, 0.0, t, (size_t)0xFFFFFFFFull, out, &p) == CSSM_EINVAL_ARG && says("too many times"));
    EXPECT(cssm_simulate_plan(&desc, 5, 42, nullptr, 0u, nan, t, 5, out, &p) == CSSM_EINVAL_ARG && says("t0 is not finite"));
    EXPECT(cssm_simulate_plan(&desc, 5, 42, nullptr, 0u, 1.0, t, 5, out, &p) == CSSM_EINVAL_ARG && says("is before t0"));
    const double dec[3] = {1.0, 3.0, 2.0}, nf[3] = {1.0, nan, 2.0};
    EXPECT(cssm_simulate_plan(&desc, 5, 42, nullptr, 0u, 0.0, dec, 3, out, &p) == CSSM_EINVAL_ARG && says("non-decreasing"));
    EXPECT(cssm_simulate_plan(&desc, 5, 42, nullptr, 0u, 0.0, nf, 3, out, &p) == CSSM_EINVAL_ARG && says("t[1] is not finite"));
    cssm_model_desc m = desc;
    m.obs_kind = CSSM_OBS_LGCP;
    EXPECT(cssm_simulate_plan(&m, 5, 42, nullptr, 0u, 0.0, t, 5, out, &p) == CSSM_EINVAL_ARG && says("log-Gaussian Cox"));
    leaves[0].has_scale = 0;
    const int kinds[5] = {CSSM_OBS_GAUSSIAN, CSSM_OBS_NEGBIN, CSSM_OBS_ZIP, CSSM_OBS_STUDENT_T, CSSM_OBS_BETA};
    const char* words[5] = {"Must provide SD parameter", "Negativebinomial", "zero inflated Poisson", "Student T Model", "Beta Model"};
    for (int i = 0; i < 5; ++i) {
      m.obs_kind = kinds[i]; m.obs_df = 3;
      EXPECT(cssm_simulate_plan(&m, 5, 42, nullptr, 0u, 0.0, t, 5, out, &p) == CSSM_EINVAL_ARG && says(words[i]));
    }
    leaves[0].has_scale = 1;
    m.obs_kind = CSSM_OBS_STUDENT_T; m.obs_df = 0;
    EXPECT(cssm_simulate_plan(&m, 5, 42, nullptr, 0u, 0.0, t, 5, out, &p) == CSSM_EINVAL_ARG && says("df >= 1"));
    m.obs_df = 3;
    EXPECT(cssm_simulate_plan(&m, 5, 42, nullptr, 0u, 0.0, t, 5, out, &p) == CSSM_OK && p.op.df == 3 && p.op.p0 == std::exp(-1.0));
    m.n_leaves = 0;
    EXPECT(cssm_simulate_plan(&m, 5, 42, nullptr, 0u, 0.0, t, 5, out, &p) == CSSM_EINVAL_DESC);
  }
  // the launch sizes
  EXPECT(cssm_simulate_rows_per_launch(3, 1u << 20, 25, 0, (size_t)1 << 30) == 21);
  EXPECT(cssm_simulate_rows_per_launch(3, 4, 25, 0, (size_t)1 << 30) == 25 && cssm_simulate_rows_per_launch(3, 4, 25, 2, (size_t)1 << 30) == 2);
  EXPECT(cssm_simulate_rows_per_launch(16, 0xffff0000ull, 25, 0, (size_t)1 << 30) == 1 && cssm_simulate_rows_per_launch(3, 4, 25, 99, 1) == 25);
  EXPECT(out[0] == 0.0);
  std::printf(failures ? "simulate_plan: %d expectation(s) failed\n" : "simulate_plan: ok\n", failures);
  return failures ? 1 : 0;
}
