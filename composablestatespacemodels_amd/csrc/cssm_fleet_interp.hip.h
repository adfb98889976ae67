// cssm_fleet_interp.hip.h -- what the fleet's host side (cssm_fleet.hip) hands to the backward pass of cssm_fleet_interpolate
// (cssm_fleet_interp.hip: k_fleet_lineage, one workgroup per (series, row) of a chunk of series).
#pragma once

#include "cssm_fleet.hip.h"

// blocks (b, row): series b of the chunk, row < d a state component, row d eta = link(f(x, time)).  off / ser / recs / fco / out are
// the chunk's own; hist / hanc are the history k_fleet_series<D, false, true> left (FleetArgs::hist / hanc: series b owns the slices
// off[b] + b .. off[b + 1] + b).
struct FleetLinArgs {
  uint32_t n, np2;                   // particles per series; the next power of two (>= 2): the keys the block sorts in LDS
  uint32_t pairing;                  // 0: output row o summarises the cloud of time index o; 1 (CSSM_INTERP_REFERENCE_PAIRING): of T_k - o
  const double* hist;
  const uint32_t* hanc;
  const unsigned long long* off;     // [series of the chunk + 1]
  const FleetSeries* ser;            // [series of the chunk]: err != 0 -- the forward pass gave the series up, its rows read NaN
  const unsigned char* recs;         // the chunk's compact records: has_obs says whether record s resampled (ancestor slice s + 1 exists)
  const double* fco;                 // [rows of the chunk][d]: the f coefficients at the time of OUTPUT row off[b] + b + o
  double* out;                       // [rows of the chunk][d + 1][3]: mean, lower, upper
  ModelK mk;
  uint32_t lo_state, hi_state, lo_eta, hi_eta;   // sel_ranks of a state row / of the eta row
};
struct FleetLinLaunch {
  FleetLinArgs args;
  int d;
  uint32_t n_series;
  hipStream_t stream;
};
int cssm_fleet_lineage_launch(const FleetLinLaunch& l);

// cssm_fleet_step_interpolate's lineage launch (k_fleet_window): blocks (q, row), request q of the call -- series req[q].k asked for
// req[q].rows rows.  words[q][j], j < rows: the slot of the series' window that holds time index (newest - j), CSSM_FLEET_WIN_RESAMPLED set
// where a weighted record wrote it (its ancestor slice is composed; the base slice and the slices of unweighted records are walked with
// the identity).  fco[q][j][d]: F at that index's time.  out[q][j][d + 1][3], preset to NaN.
#define CSSM_FLEET_WIN_RESAMPLED 0x80000000u
struct FleetWinReq {
  uint32_t k, rows;
};
struct FleetWinArgs {
  uint32_t n, np2;
  uint32_t slices, L;                // slots per series; rows per request in words / fco / out (max_lag + 1)
  const double* ring_x;              // FleetRing::x / a as the forward launch left them
  const uint32_t* ring_a;
  const FleetWinReq* req;
  const uint32_t* words;
  const FleetSeries* ser;            // the fleet's [S]: err != 0 -- the forward launch gave the series up
  const double* fco;
  double* out;
  ModelK mk;
  uint32_t lo_state, hi_state, lo_eta, hi_eta;
};
struct FleetWinLaunch {
  FleetWinArgs args;
  int d;
  uint32_t n_req;
  hipStream_t stream;
};
int cssm_fleet_window_launch(const FleetWinLaunch& l);
