// cssm_fleet_pmmh_lgcp.hip.h -- what cssm_fleet_pmmh_chains_lgcp (include/cssm_pf.h) hands its kernel: k_fleet_pmmh_lgcp in
// cssm_fleet_pmmh_lgcp.hip, one workgroup per chain, every iteration and every event of a chain inside one launch.  The arithmetic is the
// contract's (include/cssm_numerics.h, "PMMH chains on the device: LGCP").  The chain between launches, its counters and the outputs are
// cssm_fleet_pmmh_chains's (cssm_fleet_pmmh.hip.h); the record is the part of an LGCP fleet's (cssm_fleet_lgcp.hip.h) that does not depend
// on the parameters, so a record serves every iteration.
#pragma once

#include "cssm_fleet_pmmh.hip.h"

// What the host uploads per (chain, event): 24 + 8 d bytes (32 at d = 1, 48 at d = 3, 152 at d = 16) against the LGCP fleet's 32 + 40 d.
// The resampling uniform, sampleOne's slot and the d x 4 transition coefficients over delta depend on the iteration's key or on the
// proposal: the block forms them.
struct FleetPmmhLgcpRec {
  double dt;           // delta = 10^-precision, the sub-step (0 where n_sub == 0), as cssm_build_rec writes it
  int32_t n_sub;       // ceil((t - t_prev) / delta); 0: the event repeats the time before
  uint32_t step;       // the event's index in its series (Philox counter word 2)
  uint32_t fsub_off;   // time-dependent f: where the event's n_sub x d coefficient rows start in the call's sub-step table (doubles)
  uint32_t pad_;
};   // followed by the d f coefficients at the event's time (StepRec::fco)
#define CSSM_FLEET_PMMH_LGCP_REC_BYTES(d) (sizeof(FleetPmmhLgcpRec) + (size_t)(d) * 8u)

struct FleetPmmhLgcpArgs {
  uint32_t n, n_theta;
  uint32_t it0, it1;                 // the launch runs iterations it0 .. it1 - 1 of the call ...
  uint32_t n_iters;                  // ... of n_iters: the row stride of the outputs
  uint32_t first_iter;               // the call's iteration 0 is iteration first_iter of the chain (its proposal, key and decision)
  uint32_t chol_stride;              // 0: one factor for all chains; n_theta^2: one per chain
  double delta;                      // 10^-precision as cssm_build_rec forms it: the increment of every sub-step
  double* x;                         // [S][2][D][n]: the states, ping-ponged by event parity
  double* chain;                     // [S][CSSM_FLEET_PMMH_ROW]
  uint32_t* count;                   // [S][4]
  const unsigned long long* off;     // [S + 1]
  const unsigned char* recs;         // CSSM_FLEET_PMMH_LGCP_REC_BYTES(D) each
  const double* fsub;                // the call's sub-step table (f at the sub-step times of a seasonal leaf), or null: f is the record's own
  const unsigned long long* seeds;   // [S]: the chains' user seeds
  const double* chol;                // [1 or S][n_theta][n_theta]
  const cssm_prior* priors;          // [n_theta]
  double* ll;                        // [S][n_iters]
  double* theta;                     // [S][n_iters][n_theta]
  int32_t* accepted;                 // [S][n_iters]
  double* last;                      // [S][n_iters][D]
  const double* logtab;
  ModelK mk;
  If2Map map;
};

struct FleetPmmhLgcpLaunch {
  FleetPmmhLgcpArgs args;
  uint32_t n_series;
  int d, threads;
  size_t lds;                        // 8 n_even + 4 n bytes, as k_fleet_series
  hipStream_t stream;
};
int cssm_fleet_pmmh_lgcp_launch(const FleetPmmhLgcpLaunch& l);
