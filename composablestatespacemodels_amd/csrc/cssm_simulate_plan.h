// cssm_simulate_plan.h -- the host side of SimulateData (cssm_simulate, cssm_simulate_from; include/cssm_pf.h) that needs no device:
// what is refused before the first device call, and the records of the call.  Plain C++ (cssm_simulate_plan.cpp compiles with any host
// compiler, and under sanitizers with a main of its own: tests/cpp/simulate_plan_main.cpp); cssm_simulate.hip runs the plan.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "cssm_records.h"
#include "../../include/cssm_obs_draws.h"

// The observation parameters of a draw, or the reference's exception for a model without the scale its observation needs
// (model/Model.scala:150,179,214,247,291,342) and LogGaussianCox.observation = ??? (:364), as the message of cssm_last_error: the
// forecasts, the fleet's forecasts and the simulations refuse with these words.
int cssm_obs_params_or_fail(int kind, int has_scale, double scale, int df, cssm_obs_params* op);
// Times after t_start: finite and non-decreasing (`start` names t_start in the message)
int cssm_check_times(const double* t, size_t H, double t_start, const char* start);

// One simulation as the device runs it: the model, its observation parameters, the initial-state parameters (x0 = sd0 z + m0, as
// k_init takes them) and one unweighted record per time index -- with `row0` the first one is the row at t0 itself (dt = 0, F at t0).
struct SimPlan {
  HostModel m;
  cssm_obs_params op;
  double m0[CSSM_MAX_DIM], sd0[CSSM_MAX_DIM];
  std::vector<StepRec> recs;
};
// Validate a call and build its plan.  `x`: null (cssm_simulate: the paths start from the initial draw and the plan has T + 1 records, the
// first one the row at t0) or the d x n_paths states at t0 (cssm_simulate_from: T records, the first one under step `first_step`).
// Every refusal of either call but the device's is made here.
int cssm_simulate_plan(const cssm_model_desc* desc, uint64_t n_paths, uint64_t key, const double* x, uint32_t first_step, double t0, const double* t,
                       size_t T, const double* out, SimPlan* plan);
// Time indices per launch: `asked`, or (0) as many as keep the launch's rows within `cap` bytes -- as forecast_chunks sizes its chunks;
// at least 1, at most `rows`.
size_t cssm_simulate_rows_per_launch(int d, uint64_t n_paths, size_t rows, size_t asked, size_t cap);
