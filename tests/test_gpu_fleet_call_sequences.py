"""-m gpu: ONE NativePfFleet driven through calls of different kinds and sizes -- small, larger (every grow-only staging buffer of the
fleet grows while it is in use), smaller again -- and after every call each returned array held, with assert_array_equal (NaN equals
NaN), to the same call on a FRESH fleet brought to the same state.  Fresh fleets are held to the oracle by the other
tests/test_gpu_fleet*.py files, so equality is all that is asked here: what a call returns must not depend on what the fleet's
buffers served before."""
import numpy as np
import pytest

import cases
from composablestatespacemodels_amd import _abi
from composablestatespacemodels_amd.filter import NativePfFleet
from test_gpu_fleet import SEED, ragged_c2, run_key
from test_gpu_forecast_posterior import posterior

pytestmark = pytest.mark.gpu

S = 3
OPT_FORECAST_CAP = 11                                   # CSSM_OPT_FORECAST_CAP
ROUNDS = (                                              # records, horizons and posterior rows per series
    {"T": (5, 3, 4), "H": (1, 1, 2), "M": (1, 2, 5)},
    {"T": (20, 7, 13), "H": (3, 2, 4), "M": (8, 3, 12)},
    {"T": (2, 1, 2), "H": (1, 0, 1), "M": (2, 1, 1)},
)
CUM = np.cumsum([0.5, 0.0, 1.25, 1.25])                 # a forecast's horizons behind its origin (equal times: a dt = 0 step)


def series_data(k, T, r):
    """series k of round r: a time step, an origin and counts of its own; every third record from the second on is missing"""
    t, y, has = cases.poisson_counts(T, seed=SEED + 10 * r + k, dt=(1, .5, .25)[k])
    has = np.ones(T, dtype=np.uint8)
    has[1::3] = 0
    return t + 3.0 * k, y, has


def without(datas, k):
    """the same call with series k empty"""
    return [d if j != k else (np.zeros(0), np.zeros(0), np.zeros(0, dtype=np.uint8)) for j, d in enumerate(datas)]


def kib(nbytes):
    return -(-int(nbytes) // 1024)


def the_calls(model, d, n):
    """[(name, call(fleet) -> what it returns, moves, resets)]: `moves` -- the call changes the clouds or clocks of the fleet; `resets`
    -- it draws every series' cloud anew, so that nothing before it bears on the fleet's state"""
    calls = []
    for r, rnd in enumerate(ROUNDS):
        T, H, M = rnd["T"], rnd["H"], rnd["M"]
        datas = [series_data(k, T[k], r) for k in range(S)]
        end = [float(dd[0][-1]) for dd in datas]
        times = [end[k] + CUM[:H[k]] for k in range(S)]
        fkeys = [run_key(SEED + 7 * r, 100 + k) for k in range(S)]
        post = [posterior(model, M[k], seed=3 + 10 * r + k) for k in range(S)]
        # two chunks of series each: the samples of series 0 and 1 fit the cap (a row of them: (d + 3) N doubles), series 2's do not;
        # the lineage history of series 0 and 1 fits ((T_k + 1) N (8 d + 4) bytes each), series 2's does not
        fc_cap = kib((H[0] + H[1]) * (d + 3) * n * 8)
        ip_datas = without(datas, 1) if r == 1 else datas
        ip_cap = kib(sum((len(ip_datas[k][0]) + 1) * n * (8 * d + 4) for k in (0, 1)))
        active = np.array([1, 0, 1], dtype=np.uint8) if r == 1 else None
        steps = [([end[k] + (i + 1) * 0.5 for k in range(S)], [float((k + i + r) % 4) for k in range(S)], [1, (i + r) % 2, 1]) for i in range(3)]

        def forecast(fl, times=times, fkeys=fkeys, cap=fc_cap):
            fl.set_option(OPT_FORECAST_CAP, cap)
            return fl.forecast(times, fkeys, 0.9, want_samples=True)

        def interpolate(fl, datas=ip_datas, cap=ip_cap):
            fl.set_option(_abi.CSSM_OPT_INTERP_CAP, cap)
            return fl.interpolate(datas, 0.9)

        def forecast_posterior(fl, post=post, end=end, times=times, fkeys=fkeys, cap=fc_cap):
            fl.set_option(OPT_FORECAST_CAP, cap)
            return fl.forecast_posterior(post, end, times, fkeys, 0.9, want_samples=True)

        calls += [(f"round {r}: {what}", call, moves, resets) for what, call, moves, resets in (
            # (the fleet's first call: series 1 has no cloud before it and none after it)
            ("filter_intervals", lambda fl, dd=(without(datas, 1) if r == 0 else datas): fl.filter_intervals(dd, 0.9), True, r > 0),
            ("filter_forecasts", lambda fl, dd=datas: fl.filter_forecasts(dd, 0.9), True, True),
            ("filter", lambda fl, dd=datas: fl.filter(dd, want_path=True), True, True),
            ("forecast", forecast, False, False),
            ("interpolate", interpolate, False, False),
            ("forecast_posterior", forecast_posterior, False, False),
            ("ll_filter", lambda fl, dd=datas: fl.ll_filter(dd), True, True),
            ("step", lambda fl, s=steps[0], a=active: fl.step(*s, active=a), True, False),
            ("step_intervals", lambda fl, s=steps[1], a=active: fl.step_intervals(*s, active=a, interval=0.9), True, False),
            ("step_forecast", lambda fl, s=steps[2], a=active: fl.step_forecast(*s, active=a, interval=0.9), True, False),
            ("summary", lambda fl: fl.summary(0.9), False, False),
        )]
    return calls


def assert_same(got, want, where):
    if isinstance(want, dict):
        assert isinstance(got, dict) and got.keys() == want.keys(), where
        for key in want:
            assert_same(got[key], want[key], f"{where}[{key!r}]")
    elif isinstance(want, (list, tuple)):
        assert isinstance(got, (list, tuple)) and len(got) == len(want), where
        for i, (a, b) in enumerate(zip(got, want)):
            assert_same(a, b, f"{where}[{i}]")
    elif want is None:
        assert got is None, where
    else:
        np.testing.assert_array_equal(got, want, err_msg=where)


@pytest.mark.parametrize("n", [63, 100])
@pytest.mark.parametrize("name", ["c1", "c2"])
def test_one_fleet_through_calls_of_every_kind_equals_fresh_fleets(name, n):
    models = [cases.c1_model()] * S if name == "c1" else ragged_c2(S)[0]
    seeds = [SEED + 17 * k for k in range(S)]

    def fresh():
        fl = NativePfFleet(models[0], n, S)
        fl.set_params(models); fl.reseed(seeds)
        return fl

    with fresh() as used:
        assert used.d == (1 if name == "c1" else 3)
        before = []                                      # the calls that made the state `used` is in
        for what, call, moves, resets in the_calls(models[0], used.d, n):
            got = call(used)
            with fresh() as fl:
                for earlier in before:
                    earlier(fl)
                want = call(fl)
            assert_same(got, want, what)
            if resets:
                before = [call]
            elif moves:
                before.append(call)
