"""-m gpu: SimulateData for a whole fleet (include/cssm_pf.h: cssm_fleet_simulate; csrc/cssm_simulate.hip: k_fleet_simulate, one thread per
(series, pair of paths)).  The reference is the single call, which tests/test_gpu_simulate.py holds to the oracle: series k's block must
be cssm_simulate under its own model, key, t0 and times, bit for bit -- at ragged lengths, at every latent dimension, whatever the
chunking by series; the fleet itself must not change; a refused series must not stop the others; and what FilterFleet.simulate returns
must go into FilterFleet.llFilter as it is."""
from __future__ import annotations

import numpy as np
import pytest

import cases
from composablestatespacemodels_amd import _abi
from composablestatespacemodels_amd.filter import FilterFleet, NativePfFleet, Resampling
from composablestatespacemodels_amd.model import Model, Parameters, Sde, SdeParameter
from composablestatespacemodels_amd.simulate import SimulatedPoint, fleet_keys, sim_key, simulate
from test_gpu_fleet import _perturbed
from test_gpu_forecast import beta_scaled_model

pytestmark = pytest.mark.gpu

SEED = cases.SEED
LENGTHS = (0, 1, 5, 3)


def c2_fleet(S=4):
    um = cases.c2_unparam()
    models = [um.run(_perturbed(cases.c2_params, k + 1)) for k in range(S)]
    keys = [0xA11CE + 977 * k for k in range(S)]
    t0s = np.array([0.0, 1.5, -2.0, 10.25])[:S]
    times = [t0s[k] + np.cumsum([0.5, 0.0, 1.25, 0.75, 2.0])[:LENGTHS[k]] for k in range(S)]   # (an equal pair of times among them)
    return models, keys, t0s, times


@pytest.mark.parametrize("n_paths", [1, 3])
def test_every_series_is_the_single_call(n_paths):
    models, keys, t0s, times = c2_fleet()
    with NativePfFleet(models[0], 64, 4) as fl:          # (the fleet's own N plays no part)
        fl.set_params(models)
        rows, rc = fl.simulate(t0s, times, n_paths, keys)
        assert not rc.any(), rc
        for k in range(4):
            assert rows[k].shape == (LENGTHS[k] + 1, 6, n_paths)
            assert np.array_equal(rows[k], simulate(models[k], t0s[k], times[k], n_paths, keys[k])), k
        assert np.array_equal(rows[0][0], simulate(models[0], t0s[0], [], n_paths, keys[0])[0])     # T = 0: exactly its row at t0
        # a fleet that was never initialised served that; the default keys are cssm_pf_run_key(seed_k, 2^62 | k)
        fl.reseed([SEED + k for k in range(4)])
        assert fleet_keys(fl.seeds) == [sim_key(SEED + k, k) for k in range(4)] and len(set(fleet_keys(fl.seeds))) == 4
        again, rc = fl.simulate(t0s, times, n_paths)
        assert np.array_equal(again[2], simulate(models[2], t0s[2], times[2], n_paths, sim_key(SEED + 2, 2)))
        assert fl.simulate_last_ms() > 0.0


def test_the_fleet_is_not_touched():
    models, keys, t0s, times = c2_fleet()
    S, n = 4, 200
    datas = [cases.poisson_counts(4 + k, seed=SEED + k) for k in range(S)]
    nxt = [float(d[0][-1]) + 0.5 for d in datas]

    def stepped():
        fl = NativePfFleet(models[0], n, S)
        fl.set_params(models)
        fl.reseed([SEED + 17 * k for k in range(S)])
        fl.window(3)
        fl.init([float(d[0][0]) for d in datas])
        for s in range(4):
            fl.step_interpolate([float(d[0][s]) for d in datas], [float(d[1][s]) for d in datas], max_lag=1)
        return fl

    with stepped() as fl, stepped() as twin:
        before = ([fl.particles(k) for k in range(S)], [fl.ancestors(k) for k in range(S)], fl.summary(),
                  [fl.observation_index(k) for k in range(S)], [fl.window_depth(k) for k in range(S)])
        rows, rc = fl.simulate(t0s, times, 3, keys)
        assert not rc.any()
        after = ([fl.particles(k) for k in range(S)], [fl.ancestors(k) for k in range(S)], fl.summary(),
                 [fl.observation_index(k) for k in range(S)], [fl.window_depth(k) for k in range(S)])
        for a, b in zip(before[:2], after[:2]):
            assert all(np.array_equal(x, y) for x, y in zip(a, b))
        assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(before[2], after[2]))
        assert before[3:] == after[3:] and min(before[4]) >= 1          # (the window is open and stays as deep)
        ys = [1.0, 0.0, 3.0, 2.0]
        got, want = fl.step_interpolate(nxt, ys, max_lag=1), twin.step_interpolate(nxt, ys, max_lag=1)
        for a, b in zip(got[:3] + got[3] + got[4:], want[:3] + want[3] + want[4:]):        # ll, ess, rows_out, the six row arrays, rc
            assert np.array_equal(a, b, equal_nan=True)
        assert all(np.array_equal(fl.particles(k), twin.particles(k)) for k in range(S))


@pytest.mark.parametrize("d", range(1, 17))
def test_every_latent_dimension(d):
    model = cases.dim_model(d)
    times = [np.array([0.75, 2.0]), np.array([1.0, 1.0])]
    keys = [77 + d, 78 + d]
    with NativePfFleet(model, 8, 2) as fl:
        rows, rc = fl.simulate([0.0, 0.5], times, 1, keys)
        assert not rc.any()
        for k in range(2):
            assert np.array_equal(rows[k], simulate(model, [0.0, 0.5][k], times[k], 1, keys[k])), (d, k)


@pytest.mark.parametrize("n_paths", [3, 11, 32])
def test_chunking_by_series_does_not_show(n_paths):
    """CSSM_OPT_FORECAST_CAP at its smallest, 1 KiB, against the series' 1, 2, 6 and 4 rows of 48 n_paths bytes: at n_paths = 3 the cap
    holds 7 rows -- chunks {0, 1}, {2}, {3}; at 11 and 32 it holds one row -- a chunk per series, and every series with more than one
    row in windows of one time index with its states carried between the launches (an odd and an even count of paths)."""
    models, keys, t0s, times = c2_fleet()
    with NativePfFleet(models[0], 8, 4) as fl:
        fl.set_params(models)
        want, rc = fl.simulate(t0s, times, n_paths, keys)
        fl.set_option(_abi.CSSM_OPT_FORECAST_CAP, 1)
        got, rc2 = fl.simulate(t0s, times, n_paths, keys)
        fl.set_option(_abi.CSSM_OPT_FORECAST_CAP, 0)
        assert not rc.any() and not rc2.any()
        assert all(np.array_equal(a, b) for a, b in zip(got, want))
        assert np.array_equal(want[2], simulate(models[2], t0s[2], times[2], n_paths, keys[2]))


def test_a_refused_series_does_not_stop_the_others():
    ok = beta_scaled_model()
    bad = Model.beta(Sde.ouProcess(1)).run(Parameters.apply(None, SdeParameter.ouParameter(0.5, 0.2, 0.2, 0.5, 0.2)))   # no shape
    times = [np.array([0.5, 1.0]), np.array([0.5]), np.array([2.0, 1.0]), np.array([0.25, 0.5, 0.75])]
    with NativePfFleet(ok, 8, 4) as fl:
        fl.set_params([ok, bad, ok, ok])
        rows, rc = fl.simulate(0.0, times, 2, [5, 6, 7, 8])
        assert list(rc) == [0, _abi.CSSM_EINVAL_ARG, _abi.CSSM_EINVAL_ARG, 0]
        assert "series 1" in _abi.last_error() and "Must provide shape parameter for Beta Model" in _abi.last_error()
        assert np.isnan(rows[1]).all() and np.isnan(rows[2]).all()          # (series 2: its times decrease)
        for k in (0, 3):
            assert np.array_equal(rows[k], simulate(ok, 0.0, times[k], 2, [5, 6, 7, 8][k])), k


def test_the_fleet_filters_the_data_its_models_drew():
    """The loop closed: FilterFleet.simulate's output goes into FilterFleet.llFilter unchanged."""
    models, _, t0s, _ = c2_fleet()
    timess = [t0s[k] + 0.5 * np.arange(1, 9 + k) for k in range(4)]
    with FilterFleet(models, Resampling.systematicResampling, 256, seed=SEED) as ff:
        series = ff.simulate(t0s, timess)
        assert [len(s) for s in series] == [9 + k for k in range(4)] and all(isinstance(p, SimulatedPoint) for s in series for p in s)
        assert all(s[0].t == t0s[k] and [p.t for p in s[1:]] == list(timess[k]) for k, s in enumerate(series))
        assert all(p.observation is not None and np.isfinite(p.observation) and p.observation >= 0 for s in series for p in s)
        ll = ff.llFilter(series)
        assert ll.shape == (4,) and np.all(np.isfinite(ll))
        assert series[1][3].observation == ff.simulate(t0s, timess)[1][3].observation      # (deterministic under the fleet's seed)
