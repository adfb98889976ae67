// cssm_simulate.hip.h -- what the fleet's host side (cssm_fleet.hip: cssm_fleet_simulate) hands to the simulation kernels' translation
// unit (cssm_simulate.hip: k_fleet_simulate, one thread per (series, pair of paths), flattened over the grid).
#pragma once

#include <hip/hip_runtime.h>

#include "cssm_records.h"
#include "../../include/cssm_obs_draws.h"

// the initial-state parameters of one model, x0 = sd0 z + m0 (what k_init reads from the handle)
struct SimStart {
  double m0[CSSM_MAX_DIM], sd0[CSSM_MAX_DIM];
};

// One launch = the series k0 .. k0 + n_series - 1, of each the time indices rb .. rb + rn - 1 that it has (series k owns the time indices
// 0 .. T_k, T_k = off[k + 1] - off[k]; index 0 is its row at t0).  Thread p serves pair p % npairs of series k0 + p / npairs.
struct FleetSimArgs {
  uint64_t n;                        // paths per series
  uint32_t k0, n_series;
  uint32_t rb, rn;                   // the launch's window of time indices
  int from_carry, to_carry;          // the states before index rb come from `carry` / the states of the last index go there
  const unsigned long long* off;     // [S + 1], the fleet's
  const unsigned long long* keys;    // [S]
  const cssm_obs_params* op;         // [S]
  const SimStart* start;             // [S]
  const uint32_t* run;               // [S]: 0 = the series was refused, nothing of it is computed or written
  const unsigned char* recs;         // compact records (fleet_pack_rec): time index h of series k is record off[k] + k + h
  double* carry;                     // [n_series][d][n]
  double* out;                       // rows of [d + 3][n]; time index h of series k is row off[k] + k + h - out_r0
  unsigned long long out_r0;
  const double* logtab;
  ModelK mk;
};
int cssm_fleet_simulate_launch(int d, const FleetSimArgs& a, hipStream_t stream);   // 0, or the hipError_t of the launch
