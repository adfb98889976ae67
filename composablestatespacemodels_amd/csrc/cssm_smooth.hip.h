// cssm_smooth.hip.h -- what the single handle's host side (cssm_pf.hip: cssm_pf_smooth) hands to the backward launches of cssm_smooth.hip:
// k_smooth_tiles, blocks (tile of slots, group of trajectories), k_smooth_fold, a wave per trajectory over the tiles' partials, and
// k_smooth_rows, one workgroup per (time index, row).  EXTENSION: backward simulation (include/cssm_numerics.h, "backward simulation").
#pragma once

#include "cssm_internal.h"

#define CSSM_SMOOTH_GROUP 64u                /* trajectories a block of k_smooth_tiles serves from its staged tile (16 per wave) */

// what k_smooth_fold does with the partials of a time index (uniform over the launch)
enum SmoothFold : int {
  SMOOTH_START = 0,                          // index T: slot cssm_back_start(m, N, M) of the final filtering cloud
  SMOOTH_GEN = 1,                            // the genealogical step: i_s = j_{s+1}
  SMOOTH_LEVEL = 2,                          // level[m] = the max of the tiles' keys
  SMOOTH_SEARCH = 3,                         // the tile that holds the crossing from the tiles' sums, then its slot
};

// One time index s of the history cssm_pf_interpolate's forward pass keeps: slices are `d stride` doubles apart, a component's row
// `stride`, X = slice s, Xn = slice s + 1, A = the ancestors that resampled slice s (null: the identity), rec = record s on the device.
// traj[index][m], m < n_traj: the particle of slice `index` trajectory m passes through; row s + 1 is read, row s written.
struct SmoothArgs {
  uint32_t n, n_traj, tile, ntile, s;        // tile: slots per block tile (a multiple of 64), ntile = ceil(n / tile)
  size_t stride;
  const double* X;
  const double* Xn;
  const uint32_t* A;
  const StepRec* rec;
  uint64_t seed;                             // the handle's Philox key
  uint32_t* traj;                            // [T + 1][n_traj]
  unsigned long long* pkey;                  // [n_traj][ntile]: order keys of the tiles' largest lb
  cssm_u128* psum;                           // [n_traj][ntile]: the tiles' exact fixed-point sums of the weights
  double* level;                             // [n_traj]
  ModelK mk;
};
struct SmoothLaunch {
  SmoothArgs args;
  int d;
  hipStream_t stream;
};
int cssm_smooth_tiles_launch(const SmoothLaunch& l, int pass);   // pass 0: the level's keys, 1: the sums
int cssm_smooth_fold_launch(const SmoothLaunch& l, int mode);    // mode: SmoothFold

// blocks (index s, row): row < d a state component, row d eta = link(f(x, time)), over the n_traj particles traj names in slice s.
struct SmoothRowArgs {
  uint32_t n_traj, np2;                      // np2: the power of two >= max(n_traj, 2), the keys the block sorts in LDS
  size_t stride;
  const double* hist;
  const uint32_t* traj;
  const double* fco;                         // [T + 1][d]: the f coefficients at the time of row s
  double* out;                               // [T + 1][d + 1][3]: mean, lower, upper
  ModelK mk;
  uint32_t lo_state, hi_state, lo_eta, hi_eta;   // sel_ranks of n_traj values
};
struct SmoothRowLaunch {
  SmoothRowArgs args;
  int d;
  uint32_t rows;                             // T + 1
  hipStream_t stream;
};
int cssm_smooth_rows_launch(const SmoothRowLaunch& l);
