// cssm_simulate_lgcp_plan.h -- the host side of SimulateData.simLGCP (cssm_simulate_lgcp; include/cssm_pf.h) that needs no device: what
// is refused before the first device call, the accumulated grid times, the one set of transition coefficients (dt = delta exactly) and
// the f coefficients per grid index.  Plain C++ like cssm_simulate_plan.cpp (any host compiler; under sanitizers with a main of its own:
// tests/cpp/lgcp_plan_main.cpp); cssm_simulate_lgcp.hip runs the plan.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "cssm_records.h"
#include "../../include/cssm_obs_draws.h"

#define CSSM_LGCP_MAX_GRID ((size_t)1 << 24)     /* grid points of one call */
#define CSSM_LGCP_LAUNCH_CAP ((size_t)1 << 30)   /* bytes of grid rows one launch holds on the device (cssm_simulate's cap) */

struct LgcpSimPlan {
  HostModel m;
  double m0[CSSM_MAX_DIM], sd0[CSSM_MAX_DIM];   // x0 = sd0 z + m0, as SimPlan holds them
  double delta = 0.0;                           // Math.pow(10, -precision), model/Data.scala:169
  std::vector<double> grid_t;                   // t_0 = start, t_k = t_(k-1) + delta while t_k <= start + (end - start)
  double coef[CSSM_MAX_DIM][4];                 // cssm_sde_coef(.., delta, ..): every transition of the grid
  std::vector<double> fco;                      // f coefficients: one row of d (no seasonal leaf), else grid_t.size() rows at the t_k
  size_t fstride = 0;                           // doubles between the rows of two grid indices: 0 (one row) or d
};

// Validate a call and build its plan.  `out`: the caller's result slot (only checked for null).  Every refusal of cssm_simulate_lgcp but
// the device's is made here.
int cssm_simulate_lgcp_plan(const cssm_model_desc* desc, uint64_t n_paths, double start, double end, int precision, const void* out, LgcpSimPlan* plan);
// Paths per launch: `asked` (0: as many as keep the launch's grid rows within `cap` bytes), rounded up to whole pairs of paths (a pair
// shares its Philox blocks and its thread); at least 2, at most n_paths rounded up to even.
size_t cssm_lgcp_paths_per_launch(int d, uint64_t n_paths, size_t grid_points, size_t asked, size_t cap);
