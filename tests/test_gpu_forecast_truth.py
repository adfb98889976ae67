"""-m gpu: every forecast entry point against exact predictive distributions -- the helpers of tests/test_forecast_truth.py pointed
at the device, with the N, seeds and keys of that file's CPU cases.  The device is the oracle chain bit for bit (the parity tests
assert that), so every table printed here equals the table its CPU twin prints, and every verdict is known before a GPU is touched.

  cssm_pf_forecast              NativePf.forecast after run(), N = 2^14 + 3 (the last thread owns one particle), R = 16: every SDE kind,
                                every observation kind, C2 with missing records, the seasonal Gaussian; and right after init at d = 1..16
  cssm_pf_forecast_posterior    NativePf.forecast_posterior, M = 5 different parameter sets and states: every SDE kind, d = 1, 3, 9, 16
  cssm_fleet_forecast           one fleet of S = 10 series of 4096 particles that are the replicates (FLEET_S: settled on the CPU,
  cssm_fleet_forecast_posterior tests/test_forecast_truth.py says how), in single launches: c1, c2, linear, negbin
  cssm_fleet_filter_forecasts   every one-step-ahead row against the predictive from the filtering density before its record, the
  cssm_fleet_step_forecast      PIT counts / N against the exact P(Y < y), P(Y = y); streamed, the same rows bit for bit
  cssm_fleet_filter_intervals   the rows after every record against the grid's filtering mean and quantiles (check_filtering)

Every entry point runs its power checks once: the same device runs are REJECTED by wrong truths."""
import numpy as np
import pytest

import grid_reference as gr
import test_forecast_truth as tf
from composablestatespacemodels_amd.filter import NativePf, NativePfFleet
from test_forecast_truth import (FLEET_CASES, FLEET_N, FLEET_S, FORECAST_CASES, GRID_BUDGET, INTERVAL, KEY0, N, POSTERIOR_M, POSTERIOR_MODELS,
                                 POSTERIOR_T0, PRIOR_MODELS, R, SEED0, STATS, forecast_case, from_device, horizon_times, posterior,
                                 posterior_pairs, record_key)

pytestmark = pytest.mark.gpu
PIT = tf.PIT


# --------------------------------------------------------------------------------------------- NativePf.forecast
def device_runs(model, t, y, has, times):
    g = NativePf(model, N, SEED0)
    runs = []
    try:
        for r in range(R):
            g.reseed(SEED0 + r)
            g.run(t, y, has)
            runs.append(from_device(g.forecast(times, KEY0 + r, INTERVAL, want_samples=True), g.d))
    finally:
        g.close()
    return runs


@pytest.mark.parametrize("name", list(FORECAST_CASES))
def test_forecast_converges_to_the_exact_predictive(name):
    """cssm_pf_forecast"""
    model, t, y, has = forecast_case(name)
    times = horizon_times(t[-1], name)
    pred = gr.predictive(model, t, y, has, times, budget=GRID_BUDGET)
    runs = device_runs(model, t, y, has, times)
    print(f"\n{name}: NativePf.forecast N = {N}, R = {R}, horizons {times.tolist()}")
    tf.check_truth(name, runs, pred, N)
    if name in ("c1", "linear", "studentt", "c2"):               # every kind of power check once: link, observation noise, d = 3
        tf.check_power(name, model, runs, pred, N, t, y, has, times, FORECAST_CASES[name][2])


@pytest.mark.parametrize("name", PRIOR_MODELS)
def test_forecast_right_after_init_is_gaussian_in_closed_form(name):
    """cssm_pf_forecast from the initial cloud, d = 1..16"""
    model = tf.prior_model(name)
    times = horizon_times(0.0)
    pred = tf.prior_truth(model, times)
    g = NativePf(model, N, SEED0)
    runs = []
    try:
        for r in range(tf.SWEEP_R):
            g.reseed(SEED0 + r)
            g.init(0.0)
            runs.append(from_device(g.forecast(times, KEY0 + r, INTERVAL, want_samples=True), g.d))
    finally:
        g.close()
    print(f"\n{name}: NativePf.forecast right after init, d = {pred.d}, N = {N}, R = {tf.SWEEP_R}")
    tf.check_truth(f"prior {name}", runs, pred, N)
    tf.check_prior_power(f"prior {name}", runs, pred, N)


# --------------------------------------------------------------------------------------------- NativePf.forecast_posterior
@pytest.mark.parametrize("name", list(POSTERIOR_MODELS))
def test_forecast_posterior_converges_to_the_exact_mixture(name):
    """cssm_pf_forecast_posterior"""
    model, theta, x, times = tf.posterior_case(name)
    pred = gr.mixture_predictive(posterior_pairs(model, theta, x), POSTERIOR_T0, times)
    n = tf.posterior_n(name)
    g = NativePf(model, n, SEED0)
    try:
        runs = [from_device(g.forecast_posterior(theta, x, POSTERIOR_T0, times, KEY0 + r, INTERVAL, want_samples=True), g.d) for r in range(R)]
    finally:
        g.close()
    print(f"\n{name}: NativePf.forecast_posterior, d = {pred.d}, M = {POSTERIOR_M}, N = {n}, R = {R}")
    tf.check_truth(f"posterior {name}", runs, pred, n)
    tf.check_posterior_power(f"posterior {name}", model, theta, x, times, runs, pred, n)


@pytest.mark.parametrize("d", tf.SWEEP_DIMS)
def test_forecast_posterior_at_the_dimensions_between(d):
    """cssm_pf_forecast_posterior at the latent dimensions the models above do not have: with them, every d = 1..16"""
    model, theta, x, times = tf.sweep_case(d)
    pred = gr.mixture_predictive(posterior_pairs(model, theta, x), POSTERIOR_T0, times)
    g = NativePf(model, tf.SWEEP_N, SEED0)
    try:
        assert g.d == d
        runs = [from_device(g.forecast_posterior(theta, x, POSTERIOR_T0, times, KEY0 + r, INTERVAL, want_samples=True), g.d)
                for r in range(tf.SWEEP_R)]
    finally:
        g.close()
    print(f"\ndim{d}: NativePf.forecast_posterior, M = {POSTERIOR_M}, N = {tf.SWEEP_N}, R = {tf.SWEEP_R}")
    tf.check_truth(f"posterior dim{d}", runs, pred, tf.SWEEP_N)
    tf.check_posterior_power(f"posterior dim{d}", model, theta, x, times, runs, pred, tf.SWEEP_N)


# --------------------------------------------------------------------------------------------- NativePfFleet
def fleet_of(model):
    fl = NativePfFleet(model, FLEET_N, FLEET_S)
    fl.reseed([SEED0 + k for k in range(FLEET_S)])
    return fl


@pytest.mark.parametrize("name", FLEET_CASES)
def test_fleet_forecast_converges_to_the_exact_predictive(name):
    """cssm_fleet_forecast: every series' horizons in one launch"""
    model, t, y, has = forecast_case(name)
    times = horizon_times(t[-1], name)
    pred = gr.predictive(model, t, y, has, times, budget=GRID_BUDGET)
    with fleet_of(model) as fl:
        _, _, _, rc = fl.ll_filter([(t, y, has)] * FLEET_S)
        assert not rc.any(), rc
        rs = fl.forecast([times] * FLEET_S, [KEY0 + k for k in range(FLEET_S)], INTERVAL, want_samples=True)
        assert all(r["rc"] == 0 for r in rs)
        runs = [from_device(r, fl.d) for r in rs]
    print(f"\n{name}: NativePfFleet.forecast N = {FLEET_N}, S = {FLEET_S}")
    tf.check_truth(f"fleet {name}", runs, pred, FLEET_N)
    tf.check_power(f"fleet {name}", model, runs, pred, FLEET_N, t, y, has, times, None)


@pytest.mark.parametrize("name", FLEET_CASES)
def test_fleet_forecast_posterior_converges_to_the_exact_mixture(name):
    """cssm_fleet_forecast_posterior: every series' posterior-predictive forecast in one launch"""
    model = forecast_case(name)[0]
    theta, x = posterior(model, POSTERIOR_M)
    times = horizon_times(POSTERIOR_T0, name)
    pred = gr.mixture_predictive(posterior_pairs(model, theta, x), POSTERIOR_T0, times)
    with fleet_of(model) as fl:
        rs = fl.forecast_posterior([(theta, x)] * FLEET_S, POSTERIOR_T0, [times] * FLEET_S, [KEY0 + k for k in range(FLEET_S)], INTERVAL,
                                   want_samples=True)
        assert all(r["rc"] == 0 for r in rs)
        runs = [from_device(r, fl.d) for r in rs]
    print(f"\n{name}: NativePfFleet.forecast_posterior M = {POSTERIOR_M}, N = {FLEET_N}, S = {FLEET_S}")
    tf.check_truth(f"fleet posterior {name}", runs, pred, FLEET_N)
    tf.check_posterior_power(f"fleet posterior {name}", model, theta, x, times, runs, pred, FLEET_N)


@pytest.mark.parametrize("name", FLEET_CASES)
def test_fleet_one_step_ahead_rows_and_pit_counts(name):
    """cssm_fleet_filter_forecasts in one launch, then cssm_fleet_step_forecast streamed on a second fleet: the same rows bit for bit"""
    model, t, y, has = forecast_case(name)
    pred, pit, pit_err = tf.onestep_truth(model, t, y, has)
    keys = [[record_key(KEY0, k, s) for s in range(len(t))] for k in range(FLEET_S)]
    with fleet_of(model) as fl:
        _, _, _, fc, rc, fc_rc = fl.filter_forecasts([(t, y, has)] * FLEET_S, INTERVAL, keys)
        assert not rc.any() and not fc_rc.any(), (rc, fc_rc)
    runs = [{**{k: np.asarray(fc[j][k]) for k in STATS + PIT}, "draws": None} for j in range(FLEET_S)]
    print(f"\n{name}: NativePfFleet.filter_forecasts N = {FLEET_N}, S = {FLEET_S}")
    tab, frac = tf.check_onestep(f"fleet {name} one-step", runs, pred, pit, pit_err, has, FLEET_N)
    tf.check_onestep_power(f"fleet {name} one-step", runs, pred, frac, tab, FLEET_N)
    with fleet_of(model) as fl:
        fl.init(np.full(FLEET_S, float(np.min(t))))
        for s in range(len(t)):
            _, _, arr, rc, fc_rc = fl.step_forecast(np.full(FLEET_S, float(t[s])), np.full(FLEET_S, float(y[s])),
                                                    np.full(FLEET_S, has[s], dtype=np.uint8), None, [keys[k][s] for k in range(FLEET_S)], INTERVAL)
            assert not rc.any() and not fc_rc.any(), (s, rc, fc_rc)
            for j in range(FLEET_S):
                for k in STATS + PIT:
                    np.testing.assert_array_equal(arr[k][j], runs[j][k][s], err_msg=f"{name} record {s} series {j} {k}")


@pytest.mark.parametrize("name", FLEET_CASES)
def test_fleet_filter_intervals_match_the_grid(name):
    """cssm_fleet_filter_intervals: the row after every record against the grid's filtering distribution, as check_filtering holds one handle"""
    model, t, y, has = forecast_case(name)
    g = tf.filtering_truth(model, t, y, has)
    with fleet_of(model) as fl:
        _, _, _, rows, rc = fl.filter_intervals([(t, y, has)] * FLEET_S, INTERVAL)
        assert not rc.any(), rc
    summ = [np.array([rows[j][k][1:] for j in range(FLEET_S)]) for k in range(3)]      # (row 0 is the initial cloud)
    print(f"\n{name}: NativePfFleet.filter_intervals N = {FLEET_N}, S = {FLEET_S}")
    tf.check_filtering_rows(f"fleet {name}", summ, g)
    tf.check_filtering_power(f"fleet {name}", summ, g)
