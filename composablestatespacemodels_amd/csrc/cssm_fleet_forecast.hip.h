// cssm_fleet_forecast.hip.h -- what the fleet's host side (cssm_fleet.hip) hands to the forecast kernel's translation unit
// (cssm_fleet_forecast.hip: k_fleet_forecast and k_fleet_forecast_post, one workgroup per series, the whole chain of a series' horizons
// in one launch).
#pragma once

#include "cssm_fleet.hip.h"
#include "../../include/cssm_obs_draws.h"

// CSSM_OPT_FLEET_SELECT = 0: clouds from here on take a row's two order statistics by radix select, smaller ones by the bitonic sort.
// Beyond CSSM_FLEET_MAX_N, i.e. never: the sort is k_fleet_summary's known-good statement, and the A/B that would move this threshold
// has not been run.
#define CSSM_FLEET_SELECT_MIN_N (CSSM_FLEET_MAX_N + 1u)

// blocks = the series k0 .. k0 + n_series - 1 (a call that returns samples may run the fleet in chunks of series)
struct FleetFcArgs {
  uint32_t n, np2;                   // particles per series; the next power of two (>= 2): the keys the block sorts in LDS
  uint32_t k0;                       // series of block 0
  uint32_t select;                   // the two order statistics of a row: 0 = bitonic sort of its keys, 1 = radix select over them
  double* state;                     // [S][2][d][n]: buffer cur[k] is read, the other one holds the states between horizons
  const uint32_t* anc;               // [S][n]
  const unsigned long long* off;     // [S + 1]: series k owns the horizons (records, result rows) off[k] .. off[k + 1] - 1
  const uint32_t* cur;               // [S]: the buffer that holds the series' cloud (step & 1); > 1: the series is skipped
  const unsigned long long* keys;    // [S]: the Philox key of the series' forecast
  const cssm_obs_params* op;         // [S]: the series' observation parameters
  const unsigned char* recs;         // compact records (fleet_pack_rec), one per horizon
  double* stage;                     // [S][2][n]: eta and the observation draw of the horizon at hand
  double* out;                       // [R][d + 2][3]: mean, lower, upper per row (the d states, eta, obs)
  double* samples;                   // null, or [rows of the chunk][d + 3][n] starting at horizon samp_r0
  unsigned long long samp_r0;
  const double* logtab;
  ModelK mk;
  uint32_t lo_state, hi_state, lo_eta, hi_eta;   // sel_ranks of a state row / of the eta and obs rows
};
struct FleetFcLaunch {
  FleetFcArgs args;
  int d;
  uint32_t n_series;
  int threads;
  hipStream_t stream;
};
int cssm_fleet_forecast_launch(const FleetFcLaunch& l);

// k_fleet_forecast_post keeps the parameter sets of a pair (6 D doubles) in registers up to this latent dimension and reads them from
// the posterior rows above it (PostParams<D, REG>, cssm_posterior_move.hip.h).  0 = from the rows at every d: a thread serves several
// pairs per horizon, so a set is loaded per pair and horizon and used once either way, and held in registers it cost d = 6 .. 8 their
// 28 - 180 bytes of scratch and d <= 4 another 30 - 170 (the resource table).
#define CSSM_FLEET_POST_REG_MAX_D 0

// What cssm_fleet_forecast_posterior adds to FleetFcArgs (of which k_fleet_forecast_post does not read anc and op; cur[k] only says
// which buffer of a series is free: the other one)
struct FleetFcPost {
  const unsigned long long* moff;    // [S + 1]: series k owns the posterior pairs moff[k] .. moff[k + 1] - 1
  const double* x;                   // [M][d]: the state of every pair at its series' t0
  const double* rows;                // [M][3 d + 1]: cssm_posterior_rows (mu, phi, sigma per component, then the observation constant)
  uint32_t* picks;                   // [S][n]: the pair of every particle, within its series
  uint32_t draw;                     // 0: picks holds the caller's; 1: the first horizon draws them (cssm_posterior_pick) and writes them there
  int obs_df;
};
int cssm_fleet_forecast_post_launch(const FleetFcLaunch& l, const FleetFcPost& q);

// cssm_forecast.hip: the observation parameters of a draw, or the reference's exception for a model without the scale its
// observation needs, as the message of cssm_last_error
int cssm_obs_params_or_fail(int kind, int has_scale, double scale, int df, cssm_obs_params* op);
