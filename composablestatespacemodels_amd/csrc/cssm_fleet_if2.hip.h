// cssm_fleet_if2.hip.h -- what cssm_fleet_if2 (include/cssm_pf.h; EXTENSION: iterated filtering, IF2) hands its kernel: k_fleet_if2 in
// cssm_fleet_if2.hip, one workgroup per series, every iteration and every record of a search inside one launch.  The arithmetic is the
// contract's (include/cssm_numerics.h, "iterated filtering").
#pragma once

#include "cssm_fleet.hip.h"

// Per (series, record), what does not depend on a particle's parameters: 40 + 8 d bytes.  The transition coefficients and the density
// constants that depend on the scale are formed per particle on the device, so a record serves every iteration.
struct FleetIf2Rec {
  double y;            // as given (cssm_obs_y / cssm_obs_consts truncate it for the count models)
  double ypart;        // cssm_obs_ypart(kind, y, df)
  double ref;          // cssm_if2_level(kind, y, ., df) where the level does not depend on the particle (every kind but Gaussian and Student-t)
  double dt;
  int32_t has_obs;
  uint32_t step;       // the record's index within its series: the Philox counter word of its draws
};   // followed by d f coefficients (StepRec::fco)
#define CSSM_FLEET_IF2_REC_BYTES(d) (sizeof(FleetIf2Rec) + (size_t)(d) * 8u)

// per series, between the launches of a call
struct FleetIf2Series {
  uint32_t err;        // 0: searching; 2: no particle of some record had a usable weight (the series is over)
  uint32_t fail_iter;  // the iteration that failed
};

struct FleetIf2Args {
  uint32_t n, n_theta;
  uint32_t it0, it1;                 // the launch runs iterations it0 .. it1 - 1 of the call ...
  uint32_t n_iters;                  // ... of n_iters: the row stride of theta_mean / ll / cool
  uint32_t first_iter;               // the call's iteration 0 is iteration first_iter of the search (its key, its cooling factor)
  double* swarm;                     // [S][n_theta][n]: the swarm between iterations -- the call's input, every iteration's output
  double* theta;                     // [S][2][n_theta][n]: ping-ponged by record parity, read through the ancestors
  double* x;                         // [S][2][D][n]: the states, next to them
  FleetIf2Series* ser;               // [S]
  const unsigned long long* off;     // [S + 1]
  const unsigned char* recs;         // CSSM_FLEET_IF2_REC_BYTES(D) each
  const unsigned long long* seeds;   // [S]: the searches' user seeds (iteration m of the search runs under cssm_derive_key(seed, m + 1))
  const double* rw_sd;               // [n_theta]
  const double* cool;                // [n_iters]
  double* theta_mean;                // [S][n_iters][n_theta], preset to NaN
  double* ll;                        // [S][n_iters], preset to NaN
  double* ll_t;                      // may be null: per record, of the last iteration that ran
  int32_t* ess_t;                    // may be null
  uint32_t* anc_out;                 // may be null: [S][n], the ancestors behind the last record of iteration it1 - 1
  const double* logtab;
  double df;                         // Student-t degrees of freedom
  ModelK mk;
  If2Map map;
};

struct FleetIf2Launch {
  FleetIf2Args args;
  uint32_t n_series;
  int d, threads;
  size_t lds;                        // 8 n_even + 4 n bytes, as k_fleet_series
  hipStream_t stream;
};
int cssm_fleet_if2_launch(const FleetIf2Launch& l);
