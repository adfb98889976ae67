// cssm_fleet_smooth.hip.h -- what the fleet's host side (cssm_fleet.hip) hands to the two backward launches of cssm_fleet_smooth
// (cssm_fleet_smooth.hip): k_fleet_backsim, blocks (series of a chunk, group of trajectories), and k_fleet_smooth_rows, one workgroup
// per (series, row) of the chunk.  EXTENSION: backward simulation (include/cssm_numerics.h, "backward simulation").
#pragma once

#include "cssm_fleet.hip.h"

#define CSSM_BACKSIM_TPB 64u                 /* trajectories a block of k_fleet_backsim walks at most (16 per wave) */
#define CSSM_BACKSIM_STAGE_MAX (144u * 1024u) /* bytes of gathered means (d N 8) a block stages in LDS per time index (a CU has 160 KiB); beyond: through L2 */

// off / ser / recs are the chunk's own, hist / hanc the history k_fleet_series<D, false, true> left (series b owns the slices
// off[b] + b .. off[b + 1] + b), par the fleet's (series k0 + b: the Philox key).  traj[slice][m], m < n_traj: the particle of slice
// X_s trajectory m passes through (an index into the slice's cloud, not a slot of the filtering cloud).  A series without records or
// one the forward pass gave up writes nothing.
struct FleetBackArgs {
  uint32_t n, n_traj;
  const double* hist;
  const uint32_t* hanc;
  const unsigned long long* off;
  const FleetSeries* ser;
  const unsigned char* recs;
  const FleetPar* par;
  uint32_t k0;
  uint32_t* traj;                    // [slices of the chunk][n_traj]
  ModelK mk;
};
struct FleetBackLaunch {
  FleetBackArgs args;
  int d;
  uint32_t n_series;
  bool stage;                        // the gathered means of a time index in LDS (d n 8 bytes <= CSSM_BACKSIM_STAGE_MAX) or not: the same bits
  hipStream_t stream;
};
int cssm_fleet_backsim_launch(const FleetBackLaunch& l);

// blocks (b, row): row < d a state component, row d eta = link(f(x, time)), over the n_traj particles traj names per slice.
struct FleetSmRowArgs {
  uint32_t n, n_traj, np2;           // np2: the power of two >= max(n_traj, 2), the keys the block sorts in LDS
  const double* hist;
  const uint32_t* traj;
  const unsigned long long* off;
  const FleetSeries* ser;
  const double* fco;                 // [rows of the chunk][d]: the f coefficients at the time of row off[b] + b + s
  double* out;                       // [rows of the chunk][d + 1][3]: mean, lower, upper
  ModelK mk;
  uint32_t lo_state, hi_state, lo_eta, hi_eta;   // sel_ranks of n_traj values
};
struct FleetSmRowLaunch {
  FleetSmRowArgs args;
  int d;
  uint32_t n_series;
  hipStream_t stream;
};
int cssm_fleet_smooth_rows_launch(const FleetSmRowLaunch& l);
