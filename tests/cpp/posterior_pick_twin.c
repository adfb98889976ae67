/* posterior_pick_twin.c -- the host build of cssm_posterior_pick (include/cssm_obs_draws.h; gcc -O2 -ffp-contract=off -mfma), loaded
 * with ctypes by tests/test_forecast_posterior_host.py and tests/test_gpu_forecast_posterior.py: the pair each particle of
 * cssm_pf_forecast_posterior takes when no picks are given. */
#include <stddef.h>
#include <stdint.h>

#include "../../include/cssm_obs_draws.h"

/* out[i] = pick of particle i, i < n */
void twin_posterior_picks(uint64_t key, size_t n, uint64_t M, uint32_t* out) {
  for (size_t i = 0; i < n; ++i) out[i] = cssm_posterior_pick(key, (uint64_t)i, M);
}
