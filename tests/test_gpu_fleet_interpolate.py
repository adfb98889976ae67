"""cssm_fleet_interpolate (include/cssm_pf.h): FilterInterpolate of every series of a fleet in two launches -- per series the result of
cssm_pf_interpolate on a handle of its own.  Against the oracle's interpolate: ll and every order statistic bit for bit, the means
(plain fp64 sums in another order) within rtol 1e-12 / atol 1e-13, the tolerance of tests/test_interpolate.py for the same sums."""
import functools

import numpy as np
import pytest

import cases
from composablestatespacemodels_amd import CssmError, Data, _abi
from composablestatespacemodels_amd.filter import FilterFleet, FilterInterpolate, NativePf, NativePfFleet, Resampling
from oracle import oracle
from test_gpu_fleet import SEED, ragged_c2, run_key

pytestmark = pytest.mark.gpu


def assert_interpolation_equal(got_ll, got, want):
    """got: the six arrays of one series; want: (ll, mean, lower, upper, eta_of_mean, eta_lower, eta_upper) of the oracle or a handle"""
    assert got_ll == want[0], (got_ll, want[0])
    m, lo, hi, em, el, eu = got
    np.testing.assert_array_equal(lo, want[2])
    np.testing.assert_array_equal(hi, want[3])
    np.testing.assert_array_equal(el, want[5])
    np.testing.assert_array_equal(eu, want[6])
    np.testing.assert_allclose(m, want[1], rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(em, want[4], rtol=1e-12, atol=1e-13)
    assert np.all(np.isfinite(lo)) and np.all(np.isfinite(eu)) and np.all(np.isfinite(m))


def oracle_interpolate(model, n, seed, data, pairing=False, interval=0.975):
    return oracle.OraclePf(model.descriptor(), n, seed).interpolate(data[0], data[1], data[2], interval, pairing)


def with_gap(data, lo, hi):
    t, y, has = data
    has = has.copy(); has[lo:hi] = 0
    return t, y, has


# 1 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 63, 257, 1000, _abi.FLEET_MAX_N])
def test_ragged_fleet_equals_the_oracle_and_handles_of_its_own(n):
    S = 24
    models, seeds, datas = ragged_c2(S)
    with NativePfFleet(models[0], n, S) as fl:
        fl.set_params(models)
        for sd in (seeds, seeds[1:] + seeds[:1]):            # the same fleet again with the seeds rotated by one (buffers reused)
            fl.reseed(sd)
            for pairing in (False, True):
                ll, rows, rc = fl.interpolate(datas, 0.975, pairing)
                assert not rc.any(), rc
                for k in range(S):
                    assert rows[k][0].shape == (len(datas[k][0]) + 1, 3)
                    assert_interpolation_equal(ll[k], rows[k], oracle_interpolate(models[k], n, sd[k], datas[k], pairing))
                if n in (257, _abi.FLEET_MAX_N) and sd is seeds:
                    for k in (0, 7, 23):
                        with NativePf(models[k], n, sd[k]) as g:
                            assert_interpolation_equal(ll[k], rows[k], g.interpolate(*datas[k], 0.975, pairing))


# 2 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", list(range(1, 17)))
def test_every_latent_dimension(d):
    model = cases.dim_model(d)
    S, n = 3, 257
    seeds = [SEED + 17 * k for k in range(S)]
    datas = [with_gap(cases.poisson_counts(6, seed=SEED + k), 2, 4) for k in range(S)]
    with NativePfFleet(model, n, S) as fl:
        assert fl.d == d
        fl.reseed(seeds)
        for pairing in (False, True):
            ll, rows, rc = fl.interpolate(datas, 0.975, pairing)
            assert not rc.any(), rc
            for k in range(S):
                assert_interpolation_equal(ll[k], rows[k], oracle_interpolate(model, n, seeds[k], datas[k], pairing))


# 3 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["linear", "negbin"])
def test_other_observation_models(name):
    S, n, T = 5, 1000, 12
    if name == "linear":
        model, gen = cases.linear_model(), cases.gaussian_series
    else:
        model, gen = cases.literal_case("negbin", T)[0], cases.poisson_counts
    seeds = [SEED + 17 * k for k in range(S)]
    datas = [with_gap(gen(T, seed=SEED + k), T // 3, T // 3 + max(2, T // 5)) for k in range(S)]   # tests/test_interpolate.py::_series
    with NativePfFleet(model, n, S) as fl:
        fl.reseed(seeds)
        for pairing in (False, True):
            ll, rows, rc = fl.interpolate(datas, 0.975, pairing)
            assert not rc.any(), rc
            for k in range(S):
                assert_interpolation_equal(ll[k], rows[k], oracle_interpolate(model, n, seeds[k], datas[k], pairing))


# 4 ------------------------------------------------------------------------------------------------------------------------------
def test_edge_cases_of_the_genealogy():
    model = cases.c2_model()
    S, n = 4, 300
    seeds = [SEED + 17 * k for k in range(S)]
    t, y, has = cases.poisson_counts(9, seed=SEED)
    none_seen = (t, y, np.zeros(9, dtype=np.uint8))
    one = (np.array([2.5]), np.array([3.0]), np.ones(1, dtype=np.uint8))
    empty = (np.zeros(0), np.zeros(0), np.zeros(0, dtype=np.uint8))
    datas = [none_seen, one, empty, cases.poisson_counts(11, seed=SEED + 3, missing=0.3)]
    with NativePfFleet(model, n, S) as fl:
        fl.reseed(seeds)
        for pairing in (False, True):
            ll, rows, rc = fl.interpolate(datas, 0.975, pairing)
            assert list(rc) == [0, 0, _abi.CSSM_EINVAL_ARG, 0]
            assert ll[0] == 0.0                                # nothing was weighed: identity lineages
            for k in (0, 1, 3):
                assert_interpolation_equal(ll[k], rows[k], oracle_interpolate(model, n, seeds[k], datas[k], pairing))
            assert np.isnan(ll[2]) and rows[2][0].shape == (1, 3) and all(np.all(np.isnan(a)) for a in rows[2])
        # identity lineages: row s summarises the cloud of time index s as it was propagated -- the plain filter's clouds
        ll, rows, rc = fl.interpolate(datas)
        o = oracle.OraclePf(model.descriptor(), n, seeds[0])
        o.init(float(t[0]))
        for s in range(9):
            np.testing.assert_array_equal(rows[0][1][s], o.summary(0.975)[1])
            o.step(t[s], y[s], False)
        np.testing.assert_array_equal(rows[0][1][9], o.summary(0.975)[1])


# 5 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [100, 1000])
def test_one_series_fails_and_the_others_do_not_notice(n):
    model = cases.linear_model()
    S = 4
    seeds = [SEED + 17 * k for k in range(S)]
    datas = [cases.gaussian_series(8, seed=SEED + k) for k in range(S)]
    bad = datas[2][1].copy(); bad[3] = 1e200
    datas[2] = (datas[2][0], bad, datas[2][2])
    with pytest.raises(oracle.OracleError):                    # the premise: the oracle cannot interpolate that series either
        oracle_interpolate(model, n, seeds[2], datas[2])
    with NativePfFleet(model, n, S) as fl:
        fl.reseed(seeds)
        for pairing in (False, True):
            ll, rows, rc = fl.interpolate(datas, 0.975, pairing)
            assert list(rc) == [0, 0, _abi.CSSM_ENONFINITE, 0]
            assert np.isnan(ll[2]) and rows[2][0].shape == (9, 1) and all(np.all(np.isnan(a)) for a in rows[2])
            for k in (0, 1, 3):
                assert_interpolation_equal(ll[k], rows[k], oracle_interpolate(model, n, seeds[k], datas[k], pairing))


# 6 ------------------------------------------------------------------------------------------------------------------------------
def test_an_outlying_observation_forces_the_level_to_be_chosen_again():
    model = cases.c2_model()
    S, n, T = 3, 3000, 12
    seeds = [SEED + 17 * k for k in range(S)]
    datas = []
    for k in range(S):
        t, y, has = with_gap(cases.poisson_counts(T, seed=SEED + k), T // 3, T // 3 + max(2, T // 5))
        y = y.copy(); y[1] = 60.0
        datas.append((t, y, has))
    with NativePfFleet(model, n, S) as fl:
        fl.reseed(seeds)
        ll, rows, rc = fl.interpolate(datas)
        assert not rc.any(), rc
        for k in range(S):
            assert_interpolation_equal(ll[k], rows[k], oracle_interpolate(model, n, seeds[k], datas[k]))


# 7 ------------------------------------------------------------------------------------------------------------------------------
def _snapshot(fl, times):
    snap = []
    for k in range(fl.S):
        snap.append((fl.particles(k), fl.ancestors(k), fl.observation_index(k)))
    fc = fl.forecast(times, keys=[11 + k for k in range(fl.S)])
    return snap, fl.summary(), [{q: v for q, v in r.items() if q != "samples"} for r in fc]


def _assert_snapshots_equal(a, b):
    for (pa, aa, ia), (pb, ab, ib) in zip(a[0], b[0]):
        np.testing.assert_array_equal(pa, pb)
        np.testing.assert_array_equal(aa, ab)
        assert ia == ib
    for x, y in zip(a[1], b[1]):
        np.testing.assert_array_equal(x, y)
    for ra, rb in zip(a[2], b[2]):
        assert ra.keys() == rb.keys()
        for q in ra:
            np.testing.assert_array_equal(ra[q], rb[q])


def test_the_fleet_is_untouched():
    S, n = 6, 500
    models, seeds, datas = ragged_c2(S)
    data_a = datas
    data_b = [with_gap(cases.poisson_counts(9 + k, seed=SEED + 50 + k, dt=0.5), 3, 5) for k in range(S)]
    times = [[float(d[0][-1]) + 1.0, float(d[0][-1]) + 2.5] for d in data_a]
    nxt_t = np.array([float(d[0][-1]) + 0.5 for d in data_a]); nxt_y = np.arange(S, dtype=np.float64)
    with NativePfFleet(models[0], n, S) as fl, NativePfFleet(models[0], n, S) as twin:
        for f in (fl, twin):
            f.set_params(models); f.reseed(seeds)
            _, _, _, rc = f.ll_filter(data_a)
            assert not rc.any()
        before = _snapshot(fl, times)
        ll, rows, rc = fl.interpolate(data_b)
        assert not rc.any()
        for k in range(S):
            assert_interpolation_equal(ll[k], rows[k], oracle_interpolate(models[k], n, seeds[k], data_b[k]))
        _assert_snapshots_equal(before, _snapshot(fl, times))
        got, want = fl.step(nxt_t, nxt_y), twin.step(nxt_t, nxt_y)
        for x, y in zip(got, want):
            np.testing.assert_array_equal(x, y)
        for k in range(S):
            np.testing.assert_array_equal(fl.particles(k), twin.particles(k))
    # a fleet that was never initialised serves the call, and is no more initialised for it
    with NativePfFleet(models[0], n, S) as fl:
        fl.set_params(models); fl.reseed(seeds)
        with pytest.raises(CssmError) as e:
            fl.interpolate_last_ms()
        assert e.value.code == _abi.CSSM_ESTATE
        ll, rows, rc = fl.interpolate(data_b)
        assert not rc.any()
        for k in range(S):
            assert_interpolation_equal(ll[k], rows[k], oracle_interpolate(models[k], n, seeds[k], data_b[k]))
        with pytest.raises(CssmError) as e:
            fl.step(nxt_t, nxt_y)
        assert e.value.code == _abi.CSSM_ESTATE
        assert fl.observation_index(0) == 0


# 8 ------------------------------------------------------------------------------------------------------------------------------
def test_chunks_of_series_under_the_cap():
    S, n = 24, 1000
    models, seeds, datas = ragged_c2(S)
    per_series = [(len(d[0]) + 1) * n * (8 * 3 + 4) for d in datas]           # (T_k + 1) N (8 d + 4) bytes
    with NativePfFleet(models[0], n, S) as fl:
        fl.set_params(models); fl.reseed(seeds)
        whole = fl.interpolate(datas)
        assert not whole[2].any()
        # room for the longest series (28 rows; no three neighbours have so few): every chunk holds one or two series; then half of
        # that: one or two short ones, and every series longer than the cap runs alone
        big = max(per_series)
        for cap_kib in (-(-big // 1024), big // 2048):
            fl.set_option(_abi.CSSM_OPT_INTERP_CAP, cap_kib)
            ll, rows, rc = fl.interpolate(datas)
            np.testing.assert_array_equal(rc, whole[2])
            np.testing.assert_array_equal(ll, whole[0])
            for k in range(S):
                for a, b in zip(rows[k], whole[1][k]):
                    np.testing.assert_array_equal(a, b)
        with pytest.raises(CssmError) as e:
            fl.set_option(_abi.CSSM_OPT_INTERP_CAP, -1)
        assert e.value.code == _abi.CSSM_EINVAL_ARG and "negative" in str(e.value)
        fl.set_option(_abi.CSSM_OPT_INTERP_CAP, 0)
        ll, rows, rc = fl.interpolate(datas, reference_pairing=True)
        assert not rc.any()
        assert_interpolation_equal(ll[5], rows[5], oracle_interpolate(models[5], n, seeds[5], datas[5], True))


# 9 ------------------------------------------------------------------------------------------------------------------------------
def test_scale_more_blocks_than_the_gpu_holds():
    model = cases.c1_model()
    S, n, T = 2048, 64, 4
    keys = [run_key(SEED, k) for k in range(S)]
    datas = [cases.poisson_counts(T, seed=SEED + k, missing=0.3) for k in range(S)]
    with NativePfFleet(model, n, S) as fl:
        fl.reseed(keys)
        ll, rows, rc = fl.interpolate(datas)
        assert not rc.any()
        for k in range(0, S, 128):
            assert_interpolation_equal(ll[k], rows[k], oracle_interpolate(model, n, keys[k], datas[k]))
        ms = fl.interpolate_last_ms()
        assert len(ms) == 2 and ms[0] >= 0.0 and ms[1] >= 0.0


# 10 -----------------------------------------------------------------------------------------------------------------------------
def test_filter_fleet_in_the_reference_vocabulary():
    um = cases.c2_unparam()
    S, n = 3, 500
    models, _, _ = ragged_c2(S)
    datas = []
    for k in range(S):
        t, y, has = with_gap(cases.poisson_counts(8 + 2 * k, seed=SEED + k, missing=0.2), 2, 4)
        datas.append([Data(float(a), float(b) if h else None) for a, b, h in zip(t, y, has)])
    for rs in (Resampling.stratifiedResampling, Resampling.multinomialResampling):
        with pytest.raises(CssmError, match="systematic"):
            FilterFleet(models, rs, n)
    with FilterFleet(models, Resampling.systematicResampling, n, seed=SEED) as ff:
        for pairing in (False, True):
            outs = ff.interpolate(datas, 0.9, pairing)
            assert len(outs) == S
            for k in range(S):
                one = FilterInterpolate(models[k], Resampling.systematicResampling, seed=run_key(SEED, k))
                wl, wout = one.interpolate(datas[k], n, 0.9, pairing)
                gl, gout = outs[k]
                assert gl == wl and len(gout) == len(wout) == len(datas[k]) + 1
                assert gout[0].observation is None and gout[3].observation is None and gout[4].observation is None
                for a, b in zip(gout, wout):
                    assert (a.time, a.observation, a.etaIntervals, a.stateIntervals) == (b.time, b.observation, b.etaIntervals, b.stateIntervals)
                    np.testing.assert_allclose(a.state, b.state, rtol=1e-12, atol=1e-13)
                    np.testing.assert_allclose(a.eta, b.eta, rtol=1e-12, atol=1e-13)
        ms = ff.interpolate_last_ms()
        assert len(ms) == 2 and ms[0] >= 0.0 and ms[1] >= 0.0
