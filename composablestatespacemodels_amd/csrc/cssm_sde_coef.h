// cssm_sde_coef.h -- the transition coefficients of one latent component over a time step dt (model/Sde.scala:88-91,117-119,
// 139-146; :30-43 for Euler), from its constrained parameters.  One function for the host (cssm_build_rec: the per-observation
// records of the filter and of cssm_pf_forecast) and the device (k_forecast_post: a parameter set per particle), so that both
// give the same bits under the build's -ffp-contract=off.  p[0..3] as transition_one reads them (cssm_device.hip.h).
#pragma once

#include "../../include/cssm_numerics.h"
#include "../../include/cssm_pf.h"

CSSM_HD void cssm_sde_coef(int kind, double mu, double phi, double sigma, double dt, double* p) {
  p[0] = 0.0; p[1] = 0.0; p[2] = 0.0; p[3] = 0.0;
  switch (kind) {
    case CSSM_SDE_BROWNIAN: p[3] = cssm_sqrt(sigma * dt); break;
    case CSSM_SDE_GEN_BROWNIAN: p[0] = mu * dt; p[3] = cssm_sqrt(sigma * dt); break;
    case CSSM_SDE_OU: {
      const double var = (sigma * sigma / (phi * 2.0)) * (1.0 - cssm_exp(phi * -2.0 * dt));
      p[0] = mu; p[1] = cssm_exp(-phi * dt); p[3] = cssm_sqrt(var);
      break;
    }
    default: p[0] = mu; p[1] = phi; p[2] = sigma; p[3] = cssm_sqrt(dt); break;
  }
}
