/* obs_draw_twin.c -- the host build of include/cssm_obs_draws.h (gcc -O2 -ffp-contract=off -mfma), loaded with ctypes by
 * tests/test_forecast_draws.py and tests/test_gpu_forecast.py: the observation draws the device must reproduce bit for bit. */
#include <stddef.h>
#include <stdint.h>

#include "../../include/cssm_obs_draws.h"

/* cssm_obs_draw's semantics: out[i] = draw of particle gid = i at (key, step); returns cssm_obs_params_make's status */
int twin_obs_draw(int kind, const double* eta, size_t n, int has_scale, double scale, int df, uint64_t key, uint32_t step, double* out) {
  cssm_obs_params p;
  const int rc = cssm_obs_params_make(kind, has_scale, scale, df, &p);
  if (rc) return rc;
  for (size_t i = 0; i < n; ++i) {
    cssm_obs_stream s = cssm_obs_stream_at(key, (uint64_t)i, step);
    out[i] = cssm_obs_draw_one(&p, eta[i], &s, CSSM_TAB);
  }
  return 0;
}

/* one draw of particle `gid` at (key, step); *blocks_out = the Philox blocks it consumed */
double twin_obs_draw_at(int kind, double eta, int has_scale, double scale, int df, uint64_t key, uint64_t gid, uint32_t step,
                        uint32_t* blocks_out) {
  cssm_obs_params p;
  if (cssm_obs_params_make(kind, has_scale, scale, df, &p)) return cssm_nan();
  cssm_obs_stream s = cssm_obs_stream_at(key, gid, step);
  const double v = cssm_obs_draw_one(&p, eta, &s, CSSM_TAB);
  if (blocks_out) *blocks_out = s.block;
  return v;
}

/* n draws of Gamma(shape, 1), particle gid = i */
void twin_gamma(double shape, size_t n, uint64_t key, uint32_t step, double* out) {
  for (size_t i = 0; i < n; ++i) {
    cssm_obs_stream s = cssm_obs_stream_at(key, (uint64_t)i, step);
    out[i] = cssm_obs_gamma1(shape, &s, CSSM_TAB);
  }
}

/* the Poisson draw of particle gid whose stream starts at block `block` (attempt keying) */
double twin_poisson_from(double lam, uint64_t key, uint64_t gid, uint32_t step, uint32_t block) {
  cssm_obs_stream s = cssm_obs_stream_at(key, gid, step);
  s.block = block;
  return cssm_obs_poisson(lam, &s, CSSM_TAB);
}

/* PTRS's exponent log pmf(k) in its two forms (tests/test_obs_draw_laws.py holds both to mpmath over the range each serves) */
double twin_ptrs_logpmf_direct(double lam, double k) { return cssm_obs_ptrs_logpmf_direct(lam, cssm_log(lam), k); }
double twin_ptrs_logpmf_delta(double lam, double k) { return cssm_obs_ptrs_logpmf_delta(lam, k); }
