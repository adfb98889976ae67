// cssm_simulate_lgcp_plan.cpp -- host only (no HIP): the refusals, the grid and the coefficients of cssm_simulate_lgcp.  See
// cssm_simulate_lgcp_plan.h.
#include "cssm_simulate_lgcp_plan.h"

#include <algorithm>
#include <cmath>

#include "cssm_sde_coef.h"

#define fail cssm_fail

int cssm_simulate_lgcp_plan(const cssm_model_desc* desc, uint64_t n_paths, double start, double end, int precision, const void* out, LgcpSimPlan* plan) {
  if (!desc || !out || !plan) return fail(CSSM_EINVAL_ARG, "null argument");
  if (n_paths < 1 || n_paths > 0xffff0000ull) return fail(CSSM_EINVAL_ARG, "n_paths must be in [1, 2^32 - 2^16]");
  if (precision < 0 || precision > 9) return fail(CSSM_EINVAL_ARG, "precision %d out of range [0, 9]", precision);
  if (!std::isfinite(start)) return fail(CSSM_EINVAL_ARG, "start is not finite");
  if (!std::isfinite(end)) return fail(CSSM_EINVAL_ARG, "end is not finite");
  if (end < start) return fail(CSSM_EINVAL_ARG, "end = %.17g is before start = %.17g", end, start);
  if (!desc->leaves || desc->n_leaves < 1) return fail(CSSM_EINVAL_DESC, "null model descriptor");
  if (desc->obs_kind != CSSM_OBS_LGCP)
    return fail(CSSM_EINVAL_ARG, "simLGCP thins a log-Gaussian Cox process: obs_kind %d is not CSSM_OBS_LGCP (cssm_simulate draws every other model)",
                desc->obs_kind);
  int rc = cssm_build_model(&plan->m, desc, false);
  if (rc) return rc;
  const HostModel& m = plan->m;
  const int d = m.d;
  // the grid, as simSdeStream accumulates it (model/Data.scala:169-175); `precision` rules, the descriptor's lgcp_precision is the filter's
  const double delta = std::pow(10.0, -precision);
  const double span = end - start, bound = start + span;
  if (!(span / delta <= (double)CSSM_LGCP_MAX_GRID))
    return fail(CSSM_EINVAL_ARG, "too many grid points: (end - start) / 10^-%d = %.6g exceeds 2^24", precision, span / delta);
  plan->delta = delta;
  plan->grid_t.clear();
  for (double t = start; t <= bound; t = t + delta) {
    if (plan->grid_t.size() == CSSM_LGCP_MAX_GRID) return fail(CSSM_EINVAL_ARG, "too many grid points: more than 2^24 on [%.17g, %.17g] at precision %d", start, end, precision);
    plan->grid_t.push_back(t);
  }
  const size_t G1 = plan->grid_t.size();   // (>= 1: start <= start + (end - start) for end >= start)
  if (G1 * (size_t)(d + 3) * 16u > CSSM_LGCP_LAUNCH_CAP)
    return fail(CSSM_EINVAL_ARG, "the grid rows of one pair of paths (%zu grid points x %d rows) exceed the 1 GiB a launch holds", G1, d + 3);
  for (int k = 0; k < CSSM_MAX_DIM; ++k) {
    plan->m0[k] = k < d ? m.comp[k].m0 : 0.0;
    plan->sd0[k] = k < d ? std::sqrt(m.comp[k].c0) : 0.0;
    for (int q = 0; q < 4; ++q) plan->coef[k][q] = 0.0;
    if (k < d) cssm_sde_coef(m.comp[k].kind, m.comp[k].mu, m.comp[k].phi, m.comp[k].sigma, delta, plan->coef[k]);
  }
  // f at the grid times: cssm_build_rec's statements
  const size_t rows = m.lgcp_tdep ? G1 : 1;
  plan->fstride = m.lgcp_tdep ? (size_t)d : 0;
  plan->fco.assign(rows * (size_t)d, 0.0);
  for (size_t g = 0; g < rows; ++g)
    for (int k = 0; k < d; ++k) {
      const Comp& c = m.comp[k];
      double v;
      if (c.f_kind == CSSM_F_FIRST) v = (c.idx == 0) ? 1.0 : 0.0;
      else {
        double sn, cs;
        cssm_sincos2pi(cssm_seasonal_phase((double)(c.idx / 2 + 1), plan->grid_t[g], (double)c.period), &sn, &cs);
        v = (c.idx & 1) ? sn : cs;
      }
      plan->fco[g * (size_t)d + k] = v;
    }
  return CSSM_OK;
}

size_t cssm_lgcp_paths_per_launch(int d, uint64_t n_paths, size_t grid_points, size_t asked, size_t cap) {
  const size_t all = (size_t)n_paths + ((size_t)n_paths & 1u);
  size_t pc = asked ? asked : cap / ((size_t)(d + 3) * grid_points * 8u);
  pc = std::min(pc, all);
  pc = asked ? pc + (pc & 1u) : pc - (pc & 1u);   // whole pairs: a forced size rounds up, the automatic one stays within the cap
  return std::max<size_t>(2, std::min(pc, all));
}
