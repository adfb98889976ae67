// cssm_fleet_pmmh.hip.h -- what cssm_fleet_pmmh_chains (include/cssm_pf.h) hands its kernel: k_fleet_pmmh in cssm_fleet_pmmh.hip, one
// workgroup per chain, every iteration and every record of a chain inside one launch.  The arithmetic is the contract's
// (include/cssm_numerics.h, "PMMH chains on the device").  The records are cssm_fleet_if2's (FleetIf2Rec: what does not depend on the
// parameters), so a record serves every iteration.
#pragma once

#include "cssm_fleet_if2.hip.h"

// A chain between the launches of a call, [S] rows of CSSM_FLEET_PMMH_ROW(n_theta, d) doubles: cur_ll | lp_cur | cur[n_theta] |
// cur_state[d]; and [S][4] counters: accepted | proposals rejected unfiltered | proposals whose filter had no usable weight | 0.
#define CSSM_FLEET_PMMH_ROW(nt, d) (2u + (size_t)(nt) + (size_t)(d))

struct FleetPmmhArgs {
  uint32_t n, n_theta;
  uint32_t it0, it1;                 // the launch runs iterations it0 .. it1 - 1 of the call ...
  uint32_t n_iters;                  // ... of n_iters: the row stride of the outputs
  uint32_t first_iter;               // the call's iteration 0 is iteration first_iter of the chain (its proposal, key and decision)
  uint32_t chol_stride;              // 0: one factor for all chains; n_theta^2: one per chain
  double* x;                         // [S][2][D][n]: the states, ping-ponged by record parity
  double* chain;                     // [S][CSSM_FLEET_PMMH_ROW]
  uint32_t* count;                   // [S][4]
  const unsigned long long* off;     // [S + 1]
  const unsigned char* recs;         // CSSM_FLEET_IF2_REC_BYTES(D) each
  const unsigned long long* seeds;   // [S]: the chains' user seeds
  const double* chol;                // [1 or S][n_theta][n_theta]
  const cssm_prior* priors;          // [n_theta]
  double* ll;                        // [S][n_iters]
  double* theta;                     // [S][n_iters][n_theta]
  int32_t* accepted;                 // [S][n_iters]
  double* last;                      // [S][n_iters][D]
  const double* logtab;
  double df;                         // Student-t degrees of freedom
  ModelK mk;
  If2Map map;
};

struct FleetPmmhLaunch {
  FleetPmmhArgs args;
  uint32_t n_series;
  int d, threads;
  size_t lds;                        // 8 n_even + 4 n bytes, as k_fleet_series
  hipStream_t stream;
};
int cssm_fleet_pmmh_launch(const FleetPmmhLaunch& l);
