// cssm_simulate_plan.cpp -- host only (no HIP): the refusals and the records of cssm_simulate / cssm_simulate_from, and the two checks
// they share with the forecasts (the observation parameters a model draws with, the times of a call).  See cssm_simulate_plan.h.
#include "cssm_simulate_plan.h"

#include <algorithm>
#include <cmath>

#define fail cssm_fail

int cssm_obs_params_or_fail(int kind, int has_scale, double scale, int df, cssm_obs_params* op) {
  const int rc = cssm_obs_params_make(kind, has_scale, scale, df, op);
  if (rc == 0) return CSSM_OK;
  if (rc == -1) {
    const char* what = "";
    switch (kind) {
      case CSSM_OBS_GAUSSIAN: what = "Must provide SD parameter for LinearModel / No SD parameter provided to SeasonalModel"; break;
      case CSSM_OBS_NEGBIN: what = "No scale parameter provided to Negativebinomial Model"; break;
      case CSSM_OBS_ZIP: what = "Must provide probability parameter for zero inflated Poisson Model"; break;
      case CSSM_OBS_STUDENT_T: what = "No scale parameter provided to Student T Model"; break;
      default: what = "Must provide shape parameter for Beta Model"; break;
    }
    return fail(CSSM_EINVAL_ARG, "the observation model needs the scale parameter of the leftmost leaf (the reference throws Exception(\"%s\"))", what);
  }
  if (rc == -3) return fail(CSSM_EINVAL_ARG, "Student-t observations need df >= 1 (got %d)", df);
  if (kind == CSSM_OBS_LGCP)
    return fail(CSSM_EINVAL_ARG, "a log-Gaussian Cox process has no observation distribution to draw from "
                                 "(the reference's LogGaussianCox.observation is ???: scala.NotImplementedError)");
  return fail(CSSM_EINVAL_ARG, "unknown obs_kind %d", kind);
}

int cssm_check_times(const double* t, size_t H, double t_start, const char* start) {
  for (size_t h = 0; h < H; ++h) {
    const double prev = h ? t[h - 1] : t_start;
    if (!std::isfinite(t[h])) return fail(CSSM_EINVAL_ARG, "t[%zu] is not finite", h);
    if (!(t[h] >= prev)) {
      if (h) return fail(CSSM_EINVAL_ARG, "t must be non-decreasing (t[%zu] = %.17g < %.17g)", h, t[h], prev);
      return fail(CSSM_EINVAL_ARG, "t[%zu] = %.17g is before %s %.17g", h, t[h], start, prev);
    }
  }
  return CSSM_OK;
}

int cssm_simulate_plan(const cssm_model_desc* desc, uint64_t n_paths, uint64_t key, const double* x, uint32_t first_step, double t0, const double* t,
                       size_t T, const double* out, SimPlan* plan) {
  if (!desc || !out || (T && !t)) return fail(CSSM_EINVAL_ARG, "null argument");
  if (n_paths < 1 || n_paths > 0xffff0000ull) return fail(CSSM_EINVAL_ARG, "n_paths must be in [1, 2^32 - 2^16]");
  if (!x && T >= 0xffffffffull) return fail(CSSM_EINVAL_ARG, "too many times (the row at t0 draws its observation under step 2^32 - 1)");
  if (x && (uint64_t)first_step + (uint64_t)T > 0xffffffffull)
    return fail(CSSM_EINVAL_ARG, "too many times (first_step + T must not pass 2^32 - 1, the step of the row at t0)");
  if (!desc->leaves || desc->n_leaves < 1) return fail(CSSM_EINVAL_DESC, "null model descriptor");
  // (first, so that a model without the scale its observation needs is refused in the forecasts' words, the reference's exception named,
  // whatever its observation model: descriptor validation refuses some of them too, in words of its own)
  int rc = cssm_obs_params_or_fail(desc->obs_kind, desc->leaves[0].has_scale, desc->leaves[0].scale, desc->obs_df, &plan->op);
  if (rc) return rc;
  rc = cssm_build_model(&plan->m, desc, false);
  if (rc) return rc;
  HostModel& m = plan->m;
  m.n_global = n_paths; m.seed = key;
  if (!std::isfinite(t0)) return fail(CSSM_EINVAL_ARG, "t0 is not finite");
  rc = cssm_check_times(t, T, t0, "t0 =");
  if (rc) return rc;
  if (x)
    for (int k = 0; k < m.d; ++k)
      for (uint64_t i = 0; i < n_paths; ++i)
        if (!std::isfinite(x[(size_t)k * n_paths + i])) return fail(CSSM_EINVAL_ARG, "x: component %d of path %llu is not finite", k, (unsigned long long)i);
  for (int k = 0; k < CSSM_MAX_DIM; ++k) {
    plan->m0[k] = k < m.d ? m.comp[k].m0 : 0.0;
    plan->sd0[k] = k < m.d ? std::sqrt(m.comp[k].c0) : 0.0;
  }
  const size_t lead = x ? 0 : 1;
  plan->recs.resize(T + lead);
  if (lead) cssm_build_rec(&m, t0, t0, 0.0, 0, CSSM_SIM_STEP_ROW0, &plan->recs[0]);
  for (size_t h = 0; h < T; ++h) cssm_build_rec(&m, h ? t[h - 1] : t0, t[h], 0.0, 0, first_step + (uint32_t)h, &plan->recs[h + lead]);
  return CSSM_OK;
}

size_t cssm_simulate_rows_per_launch(int d, uint64_t n_paths, size_t rows, size_t asked, size_t cap) {
  size_t hc = asked ? asked : cap / ((size_t)(d + 3) * (size_t)n_paths * 8u);
  return std::max<size_t>(1, std::min(hc, rows));
}
