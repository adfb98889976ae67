"""-m gpu: forecasts of a whole fleet in one launch (include/cssm_pf.h: cssm_fleet_forecast; csrc/cssm_fleet_forecast.hip:
k_fleet_forecast, one workgroup per series).  Per series the result must be that of cssm_pf_forecast on a handle of its own, and so of
the oracle chain plus the twin draws of tests/test_gpu_forecast.py, started from fl.particles(k) at the series' clock under models[k]
and keys[k]: samples and order statistics bit for bit (== / assert_array_equal), the means to check_forecast's rtol = 1e-12,
atol = 1e-13 (plain fp64 sums in another order).  No series is skipped or excused."""
import ctypes as C

import numpy as np
import pytest

import cases
from composablestatespacemodels_amd import CssmError, Data, _abi
from composablestatespacemodels_amd.filter import Filter, FilterFleet, NativePf, NativePfFleet, ParticleFilter, Resampling
from oracle import oracle
from test_forecast_draws import build_twin
from test_gpu_fleet import _GEN, _perturbed, ragged_c2, run_key
from test_gpu_forecast import beta_scaled_model, check_forecast, expected, horizon_times

pytestmark = pytest.mark.gpu

SEED = cases.SEED
KEY = 0xF1EE7F0CA57
STAT = ("state_mean", "state_lower", "state_upper", "eta_mean", "eta_lower", "eta_upper", "obs_mean", "obs_lower", "obs_upper")


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    return build_twin(tmp_path_factory.mktemp("twin"))


def fc_key(k):
    return run_key(KEY, k)


def held_to_the_oracle(fl, k, model, clock, times, r, twin, interval=0.975):
    """series k's forecast `r` against the oracle chain + twin draws from its cloud; returns the expected arrays"""
    assert r["rc"] == 0, (k, r["rc"])
    exp = expected(model, fl.particles(k), float(clock), np.asarray(times, dtype=np.float64), r["key"], twin)
    assert r["state_mean"].shape == (len(times), fl.d) and r["samples"].shape == (len(times), fl.d + 3, fl.n)
    check_forecast(r, *exp, interval=interval)
    return exp


def all_nan(r):
    return all(np.isnan(r[name]).all() for name in STAT) and (r["samples"] is None or np.isnan(r["samples"]).all())


def equal_bits(a, b):
    for name in STAT + ("samples",):
        np.testing.assert_array_equal(a[name], b[name], err_msg=name)


# 1 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 63, 100, 1000, _abi.FLEET_MAX_N])
def test_ragged_fleet_forecasts_equal_the_oracle_and_handles_of_their_own(n, twin):
    """clamped ranks (1), a pair (2), an odd sub-wave cloud (63), padding to a power of two (100, 1000), the LDS maximum (4096);
    1 .. 5 horizons per series (equal times: a dt = 0 step), none for every sixth"""
    S = 24
    models, seeds, datas = ragged_c2(S)
    clock = [float(d[0][-1]) for d in datas]
    times = [horizon_times(clock[k])[:1 + k % 5] if k % 6 != 5 else (None if k % 12 == 5 else np.zeros(0)) for k in range(S)]
    keys = [fc_key(k) for k in range(S)]
    with NativePfFleet(models[0], n, S) as fl:
        fl.set_params(models); fl.reseed(seeds)
        _, _, _, rc = fl.ll_filter(datas)
        assert not rc.any(), rc
        exp, first = {}, {}
        for interval, how in ((0.975, 1), (0.5, 2), (0.975, 2), (0.5, 1)):      # CSSM_OPT_FLEET_SELECT: the bitonic sort, the radix select
            fl.set_option(12, how)
            rs = fl.forecast(times, keys, interval, want_samples=True)
            if (interval, how) in ((0.975, 2), (0.5, 1)):      # the other way to the same order statistics: the same bits
                for k in range(S):
                    equal_bits(rs[k], first[interval][k])
                continue
            first[interval] = rs
            assert len(rs) == S
            for k in range(S):
                if k % 6 == 5:
                    assert rs[k]["rc"] == 0 and rs[k]["state_mean"].shape == (0, fl.d) and rs[k]["samples"].shape[0] == 0
                    continue
                assert rs[k]["key"] == keys[k]
                if k not in exp:
                    exp[k] = held_to_the_oracle(fl, k, models[k], clock[k], times[k], rs[k], twin, interval)
                else:
                    check_forecast(rs[k], *exp[k], interval=interval)
                if n in (100, _abi.FLEET_MAX_N):
                    with NativePf(models[k], n, seeds[k]) as g:
                        g.run(*datas[k])
                        own = g.forecast(times[k], keys[k], interval, want_samples=True)
                    np.testing.assert_array_equal(rs[k]["samples"], own["samples"])
                    for name in STAT:
                        if name.endswith("_mean"):
                            np.testing.assert_allclose(rs[k][name], own[name], rtol=1e-12, atol=1e-13, err_msg=name)
                        else:
                            np.testing.assert_array_equal(rs[k][name], own[name], err_msg=name)


# 2 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in cases.GOLDEN_NAMES if n != "c4"] + ["gbsg", "euler", "beta_scaled"])
def test_every_served_observation_model(name, twin):
    S, n, T, H = 5, 1000, 6, 5
    model = beta_scaled_model() if name == "beta_scaled" else cases.literal_case(name, T)[0]
    gen = cases.unit_interval_series if name == "beta_scaled" else _GEN[name]
    seeds = [SEED + 17 * k for k in range(S)]
    datas = [gen(T, seed=SEED + k) for k in range(S)]
    times = [horizon_times(float(d[0][-1]))[:H] for d in datas]
    with NativePfFleet(model, n, S) as fl:
        fl.reseed(seeds)
        _, _, _, rc = fl.ll_filter(datas)
        assert not rc.any(), rc
        rs = fl.forecast(times, [fc_key(k) for k in range(S)], want_samples=True)
        if name == "beta":
            # BetaModel without a shape: the filter runs, the observation cannot be drawn (the reference throws) -- every series is
            # refused with its own status and the first one's message, and the call itself succeeds
            assert [r["rc"] for r in rs] == [_abi.CSSM_EINVAL_ARG] * S and all(all_nan(r) for r in rs)
            msg = fl.lib.cssm_last_error()
            assert b"series 0" in msg and b"Must provide shape parameter for Beta Model" in msg
            return
        for k in range(S):
            held_to_the_oracle(fl, k, model, datas[k][0][-1], times[k], rs[k], twin)
            assert np.all(np.isfinite(rs[k]["samples"][:, fl.d]))      # the gamma row: f(x, t)


# 3 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", list(range(1, 17)))
def test_every_latent_dimension(d, twin):
    model = cases.dim_model(d)
    S, n, H = 3, 257, 3
    seeds = [SEED + 17 * k for k in range(S)]
    datas = [cases.poisson_counts(4, seed=SEED + k) for k in range(S)]
    times = [horizon_times(float(dd[0][-1]))[1:1 + H] for dd in datas]
    with NativePfFleet(model, n, S) as fl:
        assert fl.d == d
        fl.reseed(seeds)
        _, _, _, rc = fl.ll_filter(datas)
        assert not rc.any(), rc
        rs = fl.forecast(times, [fc_key(k) for k in range(S)], 0.9, want_samples=True)
        for k in range(S):
            held_to_the_oracle(fl, k, model, datas[k][0][-1], times[k], rs[k], twin, 0.9)


# 4 ------------------------------------------------------------------------------------------------------------------------------
def test_the_fleet_is_untouched():
    """The states between horizons live in the series' other state buffer: after a forecast everything the fleet holds reads as before,
    and the next step of every series -- whichever buffer its cloud is in -- is the oracle's."""
    model = cases.c2_model()
    S, n = 6, 1000
    seeds = [run_key(SEED, k) for k in range(S)]
    orc = [oracle.OraclePf(model.descriptor(), n, seeds[k]) for k in range(S)]
    ys = [cases.poisson_counts(6, seed=SEED + k)[1] for k in range(S)]
    clock = np.array([0.25 * k for k in range(S)])
    with NativePfFleet(model, n, S) as fl:
        fl.reseed(seeds)
        fl.init(clock)
        for k in range(S):
            orc[k].init(clock[k])
        for r in range(3):                                     # series k has seen 3, 2, 1, 3, 2, 1 observations: both parities
            active = np.array([r < 3 - k % 3 for k in range(S)], dtype=np.uint8)
            clock = clock + 0.5 * active
            y = np.array([ys[k][r] for k in range(S)])
            _, _, rc = fl.step(clock, y, None, active)
            assert not rc.any()
            for k in range(S):
                if active[k]:
                    orc[k].step(clock[k], y[k], True)
        assert [fl.observation_index(k) for k in range(S)] == [3 - k % 3 for k in range(S)]
        before = ([fl.particles(k) for k in range(S)], [fl.ancestors(k) for k in range(S)], fl.summary(0.9))
        for want_samples in (False, True):
            rs = fl.forecast([horizon_times(clock[k]) for k in range(S)], None, 0.975, want_samples)
            assert not any(r["rc"] for r in rs)
        for k in range(S):
            np.testing.assert_array_equal(fl.particles(k), before[0][k])
            np.testing.assert_array_equal(fl.ancestors(k), before[1][k])
            np.testing.assert_array_equal(fl.particles(k), orc[k].particles())
        for a, b in zip(fl.summary(0.9), before[2]):
            np.testing.assert_array_equal(a, b)
        assert [fl.observation_index(k) for k in range(S)] == [3 - k % 3 for k in range(S)]
        clock = clock + 0.75
        y = np.array([ys[k][4] for k in range(S)])
        ll, ess, rc = fl.step(clock, y)
        assert not rc.any()
        for k in range(S):
            ol, oess = orc[k].step(clock[k], y[k], True)
            assert (ll[k], ess[k]) == (ol, oess), k
            np.testing.assert_array_equal(fl.particles(k), orc[k].particles())
            np.testing.assert_array_equal(fl.ancestors(k), orc[k].ancestors())


# 5 ------------------------------------------------------------------------------------------------------------------------------
def test_streaming_default_keys_and_identity_ancestors(twin):
    model = cases.linear_model()
    S, n = 8, 300
    seeds = [run_key(SEED, k) for k in range(S)]
    lib = _abi.load_library()
    with NativePfFleet(model, n, S) as fl:
        fl.reseed(seeds)
        clock = np.array([0.5 * k for k in range(S)])
        fl.init(clock)
        times = [horizon_times(clock[k])[:3] for k in range(S)]
        rs = fl.forecast(times, want_samples=True)             # right after init: identity ancestors, buffer 0
        for k in range(S):
            assert rs[k]["key"] == fl.forecast_key(k) == int(lib.cssm_pf_run_key(seeds[k], 1 << 63))
            held_to_the_oracle(fl, k, model, clock[k], times[k], rs[k], twin)
        active = np.array([k % 2 for k in range(S)], dtype=np.uint8)
        clock = clock + 1.0 * active
        _, _, rc = fl.step(clock, cases.gaussian_series(S)[1], None, active)
        assert not rc.any()
        times = [horizon_times(clock[k])[:3] for k in range(S)]
        a = fl.forecast(times, want_samples=True)
        b = fl.forecast(times, want_samples=True)
        for k in range(S):
            assert fl.observation_index(k) == k % 2
            assert a[k]["key"] == int(lib.cssm_pf_run_key(seeds[k], (1 << 63) | (k % 2)))
            assert (a[k]["key"] == rs[k]["key"]) == (k % 2 == 0)                   # a series that moved forecasts under another key
            equal_bits(a[k], b[k])
            held_to_the_oracle(fl, k, model, clock[k], times[k], a[k], twin)
        assert len({r["key"] for r in a}) == S


# 6 ------------------------------------------------------------------------------------------------------------------------------
def test_one_series_errors_are_its_own(twin):
    model = cases.linear_model()
    S, n = 4, 100
    seeds = [SEED + 17 * k for k in range(S)]
    datas = [cases.gaussian_series(8, seed=SEED + k) for k in range(S)]
    bad = datas[2][1].copy(); bad[3] = 1e200
    datas[2] = (datas[2][0], bad, datas[2][2])
    keys = [fc_key(k) for k in range(S)]
    with NativePfFleet(model, n, S) as fresh:
        with pytest.raises(CssmError) as e:
            fresh.forecast([[1.0]] * S, keys)
        assert e.value.code == _abi.CSSM_ESTATE and "initialised" in str(e.value)
        assert all(r["rc"] == 0 for r in fresh.forecast([None] * S, keys))          # nothing asked for: nothing refused
    with NativePfFleet(model, n, S) as fl:
        fl.reseed(seeds)
        _, _, _, rc = fl.ll_filter(datas)
        assert list(rc) == [0, 0, _abi.CSSM_ENONFINITE, 0]
        clock = [float(d[0][-1]) for d in datas]
        times = [horizon_times(clock[k]) for k in range(S)]
        times[1] = np.array([clock[1] - 1.0, clock[1] + 1.0])                        # starts before the series' clock
        rs = fl.forecast(times, keys, 0.975, want_samples=True)
        assert [r["rc"] for r in rs] == [0, _abi.CSSM_EINVAL_ARG, _abi.CSSM_ESTATE, 0]
        assert all_nan(rs[1]) and all_nan(rs[2]) and rs[1]["samples"].shape == (2, fl.d + 3, n)
        for k in (0, 3):
            held_to_the_oracle(fl, k, model, clock[k], times[k], rs[k], twin)
        for spoilt in ([clock[1] + 1.0, clock[1] + 0.5], [clock[1] + 1.0, np.nan], [np.inf]):   # decreasing, not finite
            times[1] = np.array(spoilt)
            again = fl.forecast(times, keys, 0.975, want_samples=True)
            assert [r["rc"] for r in again] == [0, _abi.CSSM_EINVAL_ARG, _abi.CSSM_ESTATE, 0] and all_nan(again[1])
            equal_bits(again[0], rs[0]); equal_bits(again[3], rs[3])
        # call-level refusals carry a message and change nothing
        for interval in (0.0, 1.5):
            with pytest.raises(CssmError) as e:
                fl.forecast(times, keys, interval)
            assert e.value.code == _abi.CSSM_EINVAL_ARG and "interval" in str(e.value)
        p = lambda arr, ty: arr.ctypes.data_as(C.POINTER(ty))
        off = np.array([1, 2, 3, 4, 5], dtype=np.uint64); tt = np.full(5, clock[0] + 1.0); ky = np.array(keys, dtype=np.uint64)
        rc = np.zeros(S, dtype=np.int32)
        call = lambda o: fl.lib.cssm_fleet_forecast(fl._h, p(o, C.c_uint64), p(tt, C.c_double), p(ky, C.c_uint64), 0.975, *([None] * 10),
                                                    p(rc, C.c_int))
        assert call(off) == _abi.CSSM_EINVAL_ARG and b"off[0]" in fl.lib.cssm_last_error()
        assert call(np.array([0, 2, 1, 3, 4], dtype=np.uint64)) == _abi.CSSM_EINVAL_ARG and b"non-decreasing" in fl.lib.cssm_last_error()
        assert fl.lib.cssm_fleet_forecast(None, p(off, C.c_uint64), p(tt, C.c_double), p(ky, C.c_uint64), 0.975, *([None] * 10),
                                          p(rc, C.c_int)) == _abi.CSSM_EINVAL_ARG
        times[1] = None
        again = fl.forecast(times, keys, 0.975, want_samples=True)                   # still usable
        assert [r["rc"] for r in again] == [0, 0, _abi.CSSM_ESTATE, 0]
        equal_bits(again[0], rs[0]); equal_bits(again[3], rs[3])


# 7 ------------------------------------------------------------------------------------------------------------------------------
def test_more_blocks_than_the_gpu_holds(twin):
    model = cases.c1_model()
    S, n, H = 2500, 64, 3
    keys = [run_key(SEED, k) for k in range(S)]
    data = cases.poisson_counts(3)
    datas = [data] * S
    times = [horizon_times(float(data[0][-1]))[:H]] * S
    with NativePfFleet(model, n, S) as fl:
        fl.reseed(keys)
        _, _, _, rc = fl.ll_filter(datas)
        assert not rc.any()
        rs = fl.forecast(times, None, 0.975, want_samples=True)
        assert not any(r["rc"] for r in rs)
        for k in (0, 1, 255, 256, 1023, 1777, 2048, S - 1):
            held_to_the_oracle(fl, k, model, data[0][-1], times[k], rs[k], twin)
        stats = fl.forecast(times)                             # without samples: the same statistics
        for k in range(0, S, 97):
            for name in STAT:
                np.testing.assert_array_equal(stats[k][name], rs[k][name])


# 8 ------------------------------------------------------------------------------------------------------------------------------
def test_filter_fleet_forecast_in_the_reference_vocabulary():
    um = cases.c2_unparam()
    S, n = 2, 500
    mods = [um.run(_perturbed(cases.c2_params, k)) for k in range(S)]
    obs = [[Data(k + 0.5 * (r + 1), float((r * 3 + k) % 5)) for r in range(4)] for k in range(S)]
    times = [[3.0, 3.0, 4.5, 9.0], [4.0, 6.5]]
    with FilterFleet(mods, Resampling.systematicResampling, n, seed=SEED) as ff:
        st = ff.initialiseState([0.0, 1.0])
        for r in range(4):
            st = ff.stepFilter(st, [obs[k][r] for k in range(S)])
        outs = ff.forecast(times, 0.95)
        means = ff.getMeanForecast([3.0, 4.0], 0.95)
        seeded = ff.forecast(times, 0.95, seed=KEY)
        for k in range(S):
            f = Filter(mods[k], Resampling.systematicResampling, seed=run_key(SEED, k))
            s = f.initialiseState(n, float(k))
            for r in range(4):
                s = f.stepFilter(s, obs[k][r])
            for got, want in ((outs[k], ParticleFilter.forecast(s, mods[k], times[k], 0.95)),
                              ([means[k]], [ParticleFilter.getMeanForecast(s, mods[k], times[k][0], 0.95)]),
                              (seeded[k], ParticleFilter.forecast(s, mods[k], times[k], 0.95, seed=KEY))):
                assert len(got) == len(want)
                for a, b in zip(got, want):
                    assert (a.t, a.obsIntervals, a.etaIntervals, a.stateIntervals) == (b.t, b.obsIntervals, b.etaIntervals, b.stateIntervals)
                    np.testing.assert_allclose([a.obs, a.eta], [b.obs, b.eta], rtol=1e-12, atol=1e-13)
                    np.testing.assert_allclose(a.state, b.state, rtol=1e-12, atol=1e-13)
        assert ff.forecast([None, []]) == [[], []]
        with pytest.raises(CssmError, match="series 1"):
            ff.forecast([[5.0], [0.5]])                         # series 1: before its clock


# 9 ------------------------------------------------------------------------------------------------------------------------------
def test_samples_in_chunks_of_series_equal_the_whole():
    S, n = 24, 100
    models, seeds, datas = ragged_c2(S)
    times = [horizon_times(float(datas[k][0][-1]))[:k % 6] for k in range(S)]        # 0 .. 5 horizons
    with NativePfFleet(models[0], n, S) as fl:
        fl.set_params(models); fl.reseed(seeds)
        fl.ll_filter(datas)
        whole = fl.forecast(times, want_samples=True)
        row_kib = (fl.d + 3) * n * 8 / 1024
        for cap_kib in (int(7 * row_kib) + 1, 1):              # a few series per chunk; one series per chunk (it is never split)
            fl.set_option(11, cap_kib)
            part = fl.forecast(times, want_samples=True)
            for k in range(S):
                equal_bits(part[k], whole[k])
        with pytest.raises(CssmError):
            fl.set_option(11, -1)
        fl.set_option(11, 0)
        for how in (1, 2, 0):                                  # sort, select, by N: one answer
            fl.set_option(12, how)
            part = fl.forecast(times, want_samples=True)
            for k in range(S):
                equal_bits(part[k], whole[k])
        with pytest.raises(CssmError):
            fl.set_option(12, 3)
