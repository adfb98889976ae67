// Stand-alone driver of the host side of SimulateData.simLGCP (csrc/cssm_simulate_lgcp_plan.cpp over csrc/cssm_model.cpp): every refusal
// that is decided before the first device call, the accumulated grid point for point and the coefficients of accepted calls, for a build
// under -fsanitize=address,undefined (tests/test_simulate_lgcp_host.py compiles and runs it).  No HIP, no device.  Exit status 0 = every
// expectation held.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "cssm_sde_coef.h"
#include "cssm_simulate_lgcp_plan.h"

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

static void ou_leaf(Leaf& l, int dim, int f_kind, int period, int harmonics) {
  l.m0.assign(1, 0.1); l.c0.assign(1, 0.0); l.mu.assign(1, 0.5); l.phi.assign(1, 0.55); l.sigma.assign(1, -1.2);
  std::memset(&l.d, 0, sizeof l.d);
  l.d.sde_kind = CSSM_SDE_OU; l.d.dim = dim; l.d.f_kind = f_kind; l.d.period = period; l.d.harmonics = harmonics;
  l.d.m0 = l.m0.data(); l.d.n_m0 = 1; l.d.c0 = l.c0.data(); l.d.n_c0 = 1; l.d.mu = l.mu.data(); l.d.n_mu = 1;
  l.d.phi = l.phi.data(); l.d.n_phi = 1; l.d.sigma = l.sigma.data(); l.d.n_sigma = 1;
}

static bool says(const char* word) { return std::strstr(cssm_last_error(), word) != nullptr; }

// the grid by the reference's statement (model/Data.scala:169-175), written out here on its own
static std::vector<double> accumulate(double start, double end, int precision) {
  const double delta = std::pow(10.0, -precision);
  std::vector<double> t;
  for (double v = start; v <= start + (end - start); v = v + delta) t.push_back(v);
  return t;
}

int main() {
  Leaf a, b;
  ou_leaf(a, 1, CSSM_F_FIRST, 0, 0);
  ou_leaf(b, 2, CSSM_F_SEASONAL, 24, 1);
  cssm_leaf_desc leaves[2] = {a.d, b.d};
  cssm_model_desc l1, l3;
  std::memset(&l1, 0, sizeof l1);
  l1.n_leaves = 1; l1.obs_kind = CSSM_OBS_LGCP; l1.leaves = leaves; l1.lgcp_precision = 1;
  l3 = l1; l3.n_leaves = 2;
  void* slot = nullptr;   // stands for the caller's result slot: the plan only looks whether there is one
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();

  {  // the grid: the number of points is whatever the accumulation yields, and so is the last time
    struct Row { double start, end; int precision; size_t points; double last; };
    const Row table[7] = {{0.0, 0.3, 1, 3, 0.2},  {0.0, 1.0, 1, 11, 0.9999999999999999},  {0.0, 2.0, 1, 20, 1.9000000000000006},
                          {0.5, 2.5, 1, 20, 2.400000000000001}, {0.0, 0.5, 2, 50, 0.49000000000000027}, {0.0, 6.0, 0, 7, 6.0},
                          {0.0, 10.0, 2, 1001, 9.999999999999831}};
    for (const Row& r : table) {
      LgcpSimPlan p;
      EXPECT(cssm_simulate_lgcp_plan(&l3, 5, r.start, r.end, r.precision, &slot, &p) == CSSM_OK);
      const std::vector<double> want = accumulate(r.start, r.end, r.precision);
      EXPECT(p.grid_t.size() == r.points && p.grid_t.back() == r.last && p.grid_t.front() == r.start);
      EXPECT(want.size() == r.points && std::memcmp(want.data(), p.grid_t.data(), r.points * sizeof(double)) == 0);
      EXPECT(p.delta == std::pow(10.0, -r.precision) && p.fstride == 3 && p.fco.size() == 3 * r.points);
      // every transition uses delta itself, not a difference of accumulated times
      double c[4];
      cssm_sde_coef(CSSM_SDE_OU, p.m.comp[0].mu, p.m.comp[0].phi, p.m.comp[0].sigma, p.delta, c);
      EXPECT(std::memcmp(c, p.coef[0], sizeof c) == 0 && std::memcmp(c, p.coef[2], sizeof c) == 0 && p.coef[3][3] == 0.0);
      // f at the accumulated times: (1, cos, sin)(2 pi t_k / 24)
      for (size_t g = 0; g < r.points; ++g) {
        double sn, cs;
        cssm_sincos2pi(cssm_seasonal_phase(1.0, p.grid_t[g], 24.0), &sn, &cs);
        EXPECT(p.fco[3 * g] == 1.0 && p.fco[3 * g + 1] == cs && p.fco[3 * g + 2] == sn);
      }
    }
    LgcpSimPlan p;   // no seasonal leaf: one row of f; the descriptor's own precision is not the grid's
    EXPECT(cssm_simulate_lgcp_plan(&l1, 1, 0.0, 10.0, 2, &slot, &p) == CSSM_OK);
    EXPECT(p.grid_t.size() == 1001 && p.fstride == 0 && p.fco.size() == 1 && p.fco[0] == 1.0 && p.m.d == 1);
    EXPECT(p.m0[0] == 0.1 && p.sd0[0] == 1.0 && p.m0[1] == 0.0 && p.sd0[15] == 0.0);
    EXPECT(cssm_simulate_lgcp_plan(&l1, 1, 3.0, 3.0, 9, &slot, &p) == CSSM_OK && p.grid_t.size() == 1 && p.grid_t[0] == 3.0);   // end == start
  }
  {  // the refusals
    LgcpSimPlan p;
    EXPECT(cssm_simulate_lgcp_plan(nullptr, 5, 0.0, 1.0, 1, &slot, &p) == CSSM_EINVAL_ARG && says("null argument"));
    EXPECT(cssm_simulate_lgcp_plan(&l1, 5, 0.0, 1.0, 1, nullptr, &p) == CSSM_EINVAL_ARG && says("null argument"));
    EXPECT(cssm_simulate_lgcp_plan(&l1, 0, 0.0, 1.0, 1, &slot, &p) == CSSM_EINVAL_ARG && says("n_paths"));
    EXPECT(cssm_simulate_lgcp_plan(&l1, 0xffff0001ull, 0.0, 1.0, 1, &slot, &p) == CSSM_EINVAL_ARG && says("n_paths"));
    EXPECT(cssm_simulate_lgcp_plan(&l1, 5, 0.0, 1.0, -1, &slot, &p) == CSSM_EINVAL_ARG && says("precision"));
    EXPECT(cssm_simulate_lgcp_plan(&l1, 5, 0.0, 1.0, 10, &slot, &p) == CSSM_EINVAL_ARG && says("precision"));
    EXPECT(cssm_simulate_lgcp_plan(&l1, 5, nan, 1.0, 1, &slot, &p) == CSSM_EINVAL_ARG && says("start is not finite"));
    EXPECT(cssm_simulate_lgcp_plan(&l1, 5, 0.0, inf, 1, &slot, &p) == CSSM_EINVAL_ARG && says("end is not finite"));
    EXPECT(cssm_simulate_lgcp_plan(&l1, 5, 2.0, 1.0, 1, &slot, &p) == CSSM_EINVAL_ARG && says("is before start"));
    cssm_model_desc m = l1;
    m.obs_kind = CSSM_OBS_POISSON;
    EXPECT(cssm_simulate_lgcp_plan(&m, 5, 0.0, 1.0, 1, &slot, &p) == CSSM_EINVAL_ARG && says("cssm_simulate"));
    m = l1; m.lgcp_precision = 12;   // validated, though not used
    EXPECT(cssm_simulate_lgcp_plan(&m, 5, 0.0, 1.0, 1, &slot, &p) == CSSM_EINVAL_DESC && says("lgcp_precision"));
    m = l1; m.n_leaves = 0;
    EXPECT(cssm_simulate_lgcp_plan(&m, 5, 0.0, 1.0, 1, &slot, &p) == CSSM_EINVAL_DESC);
    EXPECT(cssm_simulate_lgcp_plan(&l1, 5, 0.0, 100.0, 9, &slot, &p) == CSSM_EINVAL_ARG && says("too many grid points"));
    EXPECT(cssm_simulate_lgcp_plan(&l1, 5, -1e308, 1e308, 0, &slot, &p) == CSSM_EINVAL_ARG && says("too many grid points"));
    // a time that delta cannot move: the accumulation would never pass `end`; the count of points stops it
    EXPECT(cssm_simulate_lgcp_plan(&l1, 5, 1e10, 1e10 + 1e-3, 9, &slot, &p) == CSSM_EINVAL_ARG && says("too many grid points"));
    // 1.2e7 grid points x (3 + 3) rows x one pair of paths x 8 bytes > 1 GiB, within 2^24 points
    EXPECT(cssm_simulate_lgcp_plan(&l3, 5, 0.0, 1.2e7, 0, &slot, &p) == CSSM_EINVAL_ARG && says("exceed the 1 GiB"));
    EXPECT(slot == nullptr);
  }
  // the launch sizes: whole pairs of paths, within the cap unless asked for
  EXPECT(cssm_lgcp_paths_per_launch(1, 5, 1001, 0, (size_t)1 << 30) == 6 && cssm_lgcp_paths_per_launch(1, 5, 1001, 2, (size_t)1 << 30) == 2);
  EXPECT(cssm_lgcp_paths_per_launch(1, 5, 1001, 3, (size_t)1 << 30) == 4 && cssm_lgcp_paths_per_launch(1, 1, 1001, 0, (size_t)1 << 30) == 2);
  EXPECT(cssm_lgcp_paths_per_launch(1, 1u << 20, 1001, 0, (size_t)1 << 30) == 33520);   // floor(2^30 / (4 x 1001 x 8)), an even number
  EXPECT(cssm_lgcp_paths_per_launch(3, 100, 11000000, 0, (size_t)1 << 30) == 2 && cssm_lgcp_paths_per_launch(1, 5, 1001, 99, (size_t)1 << 30) == 6);
  std::printf(failures ? "lgcp_plan: %d expectation(s) failed\n" : "lgcp_plan: ok\n", failures);
  return failures ? 1 : 0;
}
