// cssm_simulate.hip.h -- what the fleet's host side (cssm_fleet.hip: cssm_fleet_simulate) hands to the simulation kernels' translation
// unit (cssm_simulate.hip: k_fleet_simulate, one thread per (series, pair of paths), flattened over the grid), and what that unit
// shares with the Cox-process simulation (cssm_simulate_lgcp.hip: k_lgcp_grid): where a pair starts and how its rows go out.
#pragma once

#include <hip/hip_runtime.h>

#include "cssm_device.hip.h"
#include "cssm_records.h"
#include "../../include/cssm_obs_draws.h"

// the initial-state parameters of one model, x0 = sd0 z + m0 (what k_init reads from the handle)
struct SimStart {
  double m0[CSSM_MAX_DIM], sd0[CSSM_MAX_DIM];
};

// the pair's d + 3 rows of one time index: out[r n + i], r = the d states, gamma, eta, obs.  An even n keeps every row 16-byte aligned
// at an even path, so the pair goes out as one 16-byte store per row and a wave writes 1 KiB of consecutive bytes.
__device__ __forceinline__ void sim_store(double* __restrict__ row, uint64_t ia, bool hasb, bool vec, double va, double vb) {
  if (vec) {
    *reinterpret_cast<double2*>(row + ia) = make_double2(va, vb);
  } else {
    row[ia] = va;
    if (hasb) row[ia + 1] = vb;
  }
}

// where a pair starts: the initial draw (initialiseState, model/ParticleFilter.scala:105-108: k_init's statement) or the carried states
template <int D>
__device__ __forceinline__ void sim_begin(const SimStart& st, const double* __restrict__ carry, int from_carry, uint64_t key, uint64_t n, uint64_t i,
                                          const double* tab, double (&x)[D]) {
  if (from_carry) {
#pragma unroll
    for (int k = 0; k < D; ++k) x[k] = carry[(size_t)k * n + i];
  } else {
    double z[D];
    draw_normals<D>(key, i, 0u, CSSM_STREAM_INIT, tab, z);
#pragma unroll
    for (int k = 0; k < D; ++k) x[k] = st.sd0[k] * z[k] + st.m0[k];
  }
}

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
