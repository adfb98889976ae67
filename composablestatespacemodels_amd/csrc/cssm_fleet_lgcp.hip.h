// cssm_fleet_lgcp.hip.h -- FilterLgcp (model/ParticleFilter.scala:169-227) inside the fleet's launch: the compact record of an event and
// the sub-step walk of step 1 of k_fleet_series<D, PATH, false, false, false, false, true> (cssm_fleet.hip.h).
//
// An event is a chain of n_sub = ceil(dt / delta) dependent transitions per particle with one exp and D normals per link, so this launch
// is bound by arithmetic where the plain fleet launch is bound by memory.  The walk restates the sub-step loop of propagate_range<...,
// LGCP = true> (cssm_propagate.hip.h, which feeds the single handle's kernels and is not shared from) from the same contract functions --
// cssm_philox_draw, cssm_normal_pair64, transition, gamma_coef, gamma_of, cssm_exp -- in the same order, so a series has the bits of a
// handle of its own.
#pragma once

#include "cssm_device.hip.h"

// What the host uploads per (series, event) of an LGCP fleet: the fields of cssm_build_rec's StepRec that FilterLgcp's step reads, with
// exactly the d components in use -- 32 + 40 d bytes (72 at d = 1, 152 at d = 3, 672 at d = 16).  No y, no density constants, no
// has_obs (every record is an event and is weighed), no level (it is predicted on the device from the event before: contract v8).
struct FleetLgcpRecHead {
  double u;            // the one uniform of systematic resampling
  double dt;           // delta = 10^-precision, the sub-step (t - t_prev = 0 where n_sub == 0)
  int32_t n_sub;       // ceil((t - t_prev) / delta); 0: the event repeats the time before -- weight gamma - gamma, the state is kept
  uint32_t step;       // the event's index in its series (Philox counter word 2)
  uint32_t fsub_off;   // time-dependent f: where the event's n_sub x d coefficient rows start in the LAUNCH's sub-step table (doubles)
  uint32_t pick;       // sampleOne's slot behind this event (`filter`)
};   // followed by d x 4 transition coefficients over delta (StepRec::coef) and d f coefficients at the event's time (StepRec::fco)
#define CSSM_FLEET_LGCP_REC_BYTES(d) (sizeof(FleetLgcpRecHead) + (size_t)(d) * 40u)

// How many of a thread's particles walk the sub-steps side by side (the loop over s outside the loop over them): 1 = one after the
// other, as propagate_range does.  DESIGN.md 5b holds the A/B.
#ifndef CSSM_FLEET_LGCP_WIDTH
#define CSSM_FLEET_LGCP_WIDTH 1
#endif

// calcWeight (model/ParticleFilter.scala:193-205, :212-217) of W particles: x[r] is moved through the record's n_sub sub-steps under
// the Philox stream of particle gid[r]; lw[r] = gamma(x[r]) - hazard.  fsub: row s of the record's slice of the launch's table (f at the
// sub-step times of a seasonal leaf), or null -- f is then the record's own.
template <int D, int W>
__device__ __forceinline__ void fleet_lgcp_weigh(const ModelK& mk, const StepRec* __restrict__ rec, const double* __restrict__ fsub, uint64_t seed,
                                                 const uint32_t (&gid)[W], const double* tab, double (&x)[W][D], double (&lw)[W]) {
  const int nsub = rec->n_sub;
  if (nsub == 0) {                           // dt == 0: (x, f, f), model/ParticleFilter.scala:212-213
#pragma unroll
    for (int r = 0; r < W; ++r) {
      const double g = gamma_of<D>(mk, rec, x[r]);
      lw[r] = g - g;
    }
    return;
  }
  const double dt = rec->dt;
  const uint32_t step = rec->step;
  double haz[W], carry[W];
  uint32_t held_a[W], held_b[W];             // the second half of the Philox block in use (contract v6: a block = two pairs)
#pragma unroll
  for (int r = 0; r < W; ++r) { haz[r] = 0.0; carry[r] = 0.0; held_a[r] = 0u; held_b[r] = 0u; }
  const double* fsub_obs = (fsub != nullptr) ? fsub + rec->fsub_off : nullptr;
  for (int s = 0; s < nsub; ++s) {           // simInitStream(...).take(n), :193-194
    const double* fc = (fsub_obs != nullptr) ? fsub_obs + (size_t)s * D : rec->fco;   // f at tau_s (uniform)
#pragma unroll
    for (int r = 0; r < W; ++r) {
      double z[D];
      // normal number q = s*D + k: even q opens Box-Muller pair q>>1 (second element kept for q+1); pair P is half P & 1 of Philox
      // block P >> 1: q = 0 mod 4 draws a block, q = 2 mod 4 uses the half it kept
#pragma unroll
      for (int k = 0; k < D; ++k) {
        const uint32_t q = (uint32_t)s * D + k;
        if ((q & 1u) == 0u) {
          double z0, z1;
          if ((q & 2u) == 0u) {
            const cssm_u32x4 blk = cssm_philox_draw(seed, (uint64_t)gid[r], step, CSSM_STREAM_STEP, q >> 2);
            held_a[r] = blk.v[2]; held_b[r] = blk.v[3];
            cssm_normal_pair64(blk.v[0], blk.v[1], tab, &z0, &z1);
          } else {
            cssm_normal_pair64(held_a[r], held_b[r], tab, &z0, &z1);
          }
          z[k] = z0; carry[r] = z1;
        } else {
          z[k] = carry[r];
        }
      }
      transition<D>(mk, rec, dt, x[r], z);
      haz[r] = haz[r] + cssm_exp(gamma_coef<D>(mk, fc, x[r])) * dt;   // :203-205
    }
  }
#pragma unroll
  for (int r = 0; r < W; ++r) lw[r] = gamma_of<D>(mk, rec, x[r]) - haz[r];   // :200, :217
}
