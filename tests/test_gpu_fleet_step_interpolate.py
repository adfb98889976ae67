"""-m gpu: cssm_fleet_step_interpolate (include/cssm_pf.h) -- FilterInterpolate as the stream it is: one observation per sensor per call,
every cloud remembered in a bounded window on the device, and per call the summaries of the last lag + 1 time indices through the
lineages that survive to the cloud just written.

After the call that steps record m, row j of a series is row m + 1 - j of the interpolation of its records 0 .. m.  Two answers hold
it: the CPU oracle's ``OraclePf.interpolate`` of the prefix (ll and every order statistic bit for bit; the means -- plain fp64 sums in
another order -- within rtol 1e-12 / atol 1e-13, the tolerance of tests/test_interpolate.py for the same sums) and
``NativePfFleet.interpolate`` of the same prefix on the same fleet (it is only lent: the means bit for bit too).  Every other
comparison is == / assert_array_equal."""
import ctypes as C

import numpy as np
import pytest

import cases
from composablestatespacemodels_amd import CssmError, Data, _abi, formats
from composablestatespacemodels_amd.filter import FilterFleet, NativePfFleet, Resampling, _p
from oracle import oracle
from test_gpu_fleet import SEED, ragged_c2
from test_gpu_fleet_interpolate import oracle_interpolate, with_gap

pytestmark = pytest.mark.gpu

NO = None   # a lag of None: CSSM_FLEET_NO_ROWS


def prefix(data, m):
    """records 0 .. m - 1 of a series (at least one, at most all)"""
    m = max(1, min(m, len(data[0])))
    return data[0][:m], data[1][:m], data[2][:m]


def record(datas, m):
    """call m of a stream over ragged series: (t, y, has, active) -- a series whose data ended is inactive"""
    S = len(datas)
    act = np.array([1 if m < len(d[0]) else 0 for d in datas], dtype=np.uint8)
    t = np.array([d[0][m] if a else 0.0 for d, a in zip(datas, act)])
    y = np.array([d[1][m] if a else 0.0 for d, a in zip(datas, act)])
    has = np.array([d[2][m] if a else 0 for d, a in zip(datas, act)], dtype=np.uint8)
    assert len(t) == S
    return t, y, has, act


def assert_tail(rows, k, nrows, want, exact):
    """rows: the six arrays of a step_interpolate call; series k's rows 0 .. nrows - 1 against the LAST rows of `want` (the six arrays of
    a prefix interpolation, oldest first), newest first; the rows beyond read NaN"""
    last = len(want[3]) - 1
    for a, w, order_stat in zip(rows, want, (False, True, True, False, True, True)):
        for j in range(nrows):
            if exact or order_stat:
                np.testing.assert_array_equal(a[k, j], w[last - j], err_msg=f"series {k} row {j}")
            else:
                np.testing.assert_allclose(a[k, j], w[last - j], rtol=1e-12, atol=1e-13, err_msg=f"series {k} row {j}")
        assert np.all(np.isnan(a[k, nrows:])), (k, nrows)
        assert np.all(np.isfinite(a[k, :nrows])), (k, nrows)


def stream_and_check(fl, models, seeds, datas, slices, lag_of, max_lag, calls=None, joined_at=0):
    """Stream `datas` one record per call through step_interpolate on an initialised fleet whose window is open; after every call hold
    ll / ess to the oracle's step and the rows to both prefix interpolations.  lag_of(m): the lag of call m (for every series).
    joined_at: the records the series had seen when the window was opened (the rows never reach behind it)."""
    S, n = fl.S, fl.n
    orc = [oracle.OraclePf(models[k].descriptor(), n, seeds[k]) for k in range(S)]
    for k in range(S):
        orc[k].init(float(datas[k][0][0]))
        for m in range(joined_at):
            orc[k].step(float(datas[k][0][m]), float(datas[k][1][m]), bool(datas[k][2][m]))
    T = max(len(d[0]) for d in datas)
    for m in range(joined_at, T if calls is None else min(T, calls)):
        t, y, has, act = record(datas, m)
        lag = lag_of(m)
        depth_before = [fl.window_depth(k) for k in range(S)]
        ll, ess, nrows, rows, rc = fl.step_interpolate(t, y, has, act, [lag] * S, max_lag)
        assert not rc.any(), rc
        _, ref, rci = fl.interpolate([prefix(d, m + 1) for d in datas])       # (the fleet is only lent: mid-stream)
        assert not rci.any()
        for k in range(S):
            if not act[k]:
                assert np.isnan(ll[k]) and ess[k] == -1 and nrows[k] == 0 and all(np.all(np.isnan(a[k])) for a in rows)
                assert fl.window_depth(k) == depth_before[k]
                continue
            assert (ll[k], ess[k]) == orc[k].step(float(t[k]), float(y[k]), bool(has[k])), (k, m)
            depth = min(m + 1 - joined_at, slices - 1)
            assert fl.window_depth(k) == depth, (k, m)
            assert nrows[k] == min(lag, depth) + 1, (k, m, nrows[k])
            assert_tail(rows, k, int(nrows[k]), ref[k], exact=True)
            want = oracle_interpolate(models[k], n, seeds[k], prefix(datas[k], m + 1))
            assert ll[k] == want[0]
            assert_tail(rows, k, int(nrows[k]), want[1:], exact=False)


# 1 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 63, 257, 1000, _abi.FLEET_MAX_N])
def test_every_prefix_of_a_ragged_fleet(n):
    S, slices = 6, 4
    models, seeds, datas = ragged_c2(S)
    with NativePfFleet(models[0], n, S) as fl:
        fl.set_params(models)
        fl.window(slices)
        for sd in (seeds, seeds[1:] + seeds[:1]):            # the same fleet again with the seeds rotated by one (buffers reused)
            fl.reseed(sd)
            fl.init([float(d[0][0]) for d in datas])
            assert [fl.window_depth(k) for k in range(S)] == [0] * S
            stream_and_check(fl, models, sd, datas, slices, lambda m: m % 6, 5)   # lags 0 .. 5: beyond the depth and the window
        ms = fl.step_interpolate_last_ms()
        assert ms[0] >= 0.0 and ms[1] > 0.0


# 2 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", list(range(1, 17)))
def test_every_latent_dimension(d):
    model = cases.dim_model(d)
    S, n, slices = 3, 257, 3
    seeds = [SEED + 17 * k for k in range(S)]
    datas = [with_gap(cases.poisson_counts(6, seed=SEED + k), 2, 4) for k in range(S)]
    with NativePfFleet(model, n, S) as fl:
        assert fl.d == d
        fl.reseed(seeds)
        fl.window(slices)
        fl.init([0.0] * S)
        stream_and_check(fl, [model] * S, seeds, datas, slices, lambda m: 2, 2)


# 3 ------------------------------------------------------------------------------------------------------------------------------
def test_the_fleet_is_left_as_step_leaves_it():
    S, n = 6, 500
    models, seeds, datas = ragged_c2(S)
    with NativePfFleet(models[0], n, S) as fl, NativePfFleet(models[0], n, S) as twin:
        for f in (fl, twin):
            f.set_params(models); f.reseed(seeds)
            f.init([float(d[0][0]) for d in datas])
        fl.window(3)
        for m in range(max(len(d[0]) for d in datas)):
            t, y, has, act = record(datas, m)
            ll, ess, nrows, rows, rc = fl.step_interpolate(t, y, has, act, None, 1)
            wl, we, wrows, wrc = twin.step_intervals(t, y, has, act)
            np.testing.assert_array_equal(ll, wl); np.testing.assert_array_equal(ess, we); np.testing.assert_array_equal(rc, wrc)
            for q in (1, 2, 4, 5):                            # row 0: the cloud just written -- step_intervals' order statistics
                np.testing.assert_array_equal(rows[q][:, 0], wrows[q])
        for k in range(S):
            np.testing.assert_array_equal(fl.particles(k), twin.particles(k))
            np.testing.assert_array_equal(fl.ancestors(k), twin.ancestors(k))
            assert fl.observation_index(k) == twin.observation_index(k) == len(datas[k][0])
        nt = np.array([float(d[0][-1]) + 0.5 for d in datas]); ny = np.arange(S, dtype=np.float64)
        for a, b in zip(fl.step(nt, ny), twin.step(nt, ny)):
            np.testing.assert_array_equal(a, b)
        for k in range(S):
            np.testing.assert_array_equal(fl.particles(k), twin.particles(k))


# 4 ------------------------------------------------------------------------------------------------------------------------------
def test_joining_and_restarting():
    S, n, slices = 3, 300, 4
    model = cases.c2_model()
    seeds = [SEED + 17 * k for k in range(S)]
    datas = [cases.poisson_counts(14, seed=SEED + k, missing=0.2) for k in range(S)]
    depths = lambda f: [f.window_depth(k) for k in range(S)]

    def plain(f, lo, hi):
        for m in range(lo, hi):
            t, y, has, act = record(datas, m)
            assert not f.step(t, y, has, act)[2].any()

    with NativePfFleet(model, n, S) as fl:
        fl.reseed(seeds)
        fl.init([0.0] * S)
        with pytest.raises(CssmError) as e:                  # no window yet
            fl.step_interpolate(*record(datas, 0)[:3], max_lag=1)
        assert e.value.code == _abi.CSSM_ESTATE and "cssm_fleet_window" in str(e.value)
        with pytest.raises(CssmError) as e:
            fl.step_interpolate_last_ms()
        assert e.value.code == _abi.CSSM_ESTATE
        # joining: three plain steps, then the window -- the rows never reach behind the join and equal the prefix's
        plain(fl, 0, 3)
        fl.window(slices)
        assert depths(fl) == [0] * S
        stream_and_check(fl, [model] * S, seeds, datas, slices, lambda m: 3, 3, calls=6, joined_at=3)
        assert depths(fl) == [3] * S
        # calls that only read leave the window alone
        fl.summary(); fl.forecast([[20.0]] * S); fl.interpolate([prefix(d, 4) for d in datas])
        for k in range(S):
            fl.particles(k); fl.ancestors(k)
        assert depths(fl) == [3] * S
        # a plain step of series 0 and 2 restarts theirs; series 1 goes on
        t, y, has, _ = record(datas, 6)
        assert not fl.step(t, y, has, [1, 0, 1])[2].any()
        assert depths(fl) == [0, 3, 0]
        ll, ess, nrows, rows, rc = fl.step_interpolate(*record(datas, 7)[:3], active=[1, 0, 1], lag=[3, NO, 3], max_lag=3)
        assert list(nrows) == [2, 0, 2] and depths(fl) == [1, 3, 1]
        _, ref, _ = fl.interpolate([prefix(d, 8) for d in datas])
        for k in (0, 2):
            assert_tail(rows, k, 2, ref[k], exact=True)       # the base slice is the cloud record 6 left: row 7 of the prefix
        # init plus the same number of plain steps lands on the same observation index with a cloud of its own: the window restarts
        idx = fl.observation_index(0)
        fl.init([0.0] * S)
        assert depths(fl) == [0] * S
        plain(fl, 0, idx)
        assert fl.observation_index(0) == idx and depths(fl) == [0] * S
        stream_and_check(fl, [model] * S, seeds, datas, slices, lambda m: 3, 3, calls=idx + 2, joined_at=idx)
        assert depths(fl) == [2] * S
        # reseed and set_params restart
        fl.reseed(seeds)
        assert depths(fl) == [0] * S
        ll, ess, nrows, rows, rc = fl.step_interpolate(*record(datas, idx + 2)[:3], max_lag=3)
        assert list(nrows) == [2] * S and depths(fl) == [1] * S
        fl.set_params([model] * S)
        assert depths(fl) == [0] * S
        ll, ess, nrows, rows, rc = fl.step_interpolate(*record(datas, idx + 3)[:3], max_lag=3)
        assert list(nrows) == [2] * S
        sm = fl.summary()
        for q in (1, 2, 4, 5):                                # row 0 is the cloud the fleet holds now
            np.testing.assert_array_equal(rows[q][:, 0], sm[q])
        # closing and re-opening
        fl.window(0)
        assert depths(fl) == [0] * S
        with pytest.raises(CssmError) as e:
            fl.step_interpolate(*record(datas, idx + 4)[:3], max_lag=3)
        assert e.value.code == _abi.CSSM_ESTATE and "cssm_fleet_window" in str(e.value)
        with pytest.raises(CssmError) as e:
            fl.window(1)
        assert e.value.code == _abi.CSSM_EINVAL_ARG
        fl.window(2)
        for m in (idx + 4, idx + 5):
            ll, ess, nrows, rows, rc = fl.step_interpolate(*record(datas, m)[:3], max_lag=3)
            assert list(nrows) == [2] * S and depths(fl) == [1] * S and not rc.any()


# 5 ------------------------------------------------------------------------------------------------------------------------------
def test_per_series_lag_writes_only_what_is_asked():
    S, n, slices, L = 5, 257, 4, 4
    models, seeds, datas = ragged_c2(S)
    datas = [prefix(d, 5) for d in datas]
    with NativePfFleet(models[0], n, S) as fl, NativePfFleet(models[0], n, S) as twin:
        for f in (fl, twin):
            f.set_params(models); f.reseed(seeds)
            f.init([float(d[0][0]) for d in datas])
        fl.window(slices)
        lags = [3, NO, 0, 2, 3]
        for m in range(5):
            t, y, has, _ = record(datas, m)
            act = np.array([1, 1, 1, 1, 0], dtype=np.uint8)
            lg = fl._lags(lags, L - 1)
            ll = np.full(S, 7.5); ess = np.full(S, -7, dtype=np.int32); nrows = np.full(S, 77, dtype=np.uint32)
            rc = np.zeros(S, dtype=np.int32)
            m6 = [np.full((S, L, fl.d), 7.5) for _ in range(3)] + [np.full((S, L), 7.5) for _ in range(3)]
            _abi.check(fl.lib.cssm_fleet_step_interpolate(fl._h, _p(act, C.POINTER(C.c_uint8)), _p(t), _p(y), _p(has, C.POINTER(C.c_uint8)),
                                                          _p(lg, C.POINTER(C.c_uint32)), L - 1, 0.975, _p(ll), _p(ess, C.POINTER(C.c_int32)),
                                                          _p(nrows, C.POINTER(C.c_uint32)), *[_p(a) for a in m6], _p(rc, C.POINTER(C.c_int))))
            wl, we, wrc = twin.step(t, y, has, act)
            depth = min(m + 1, slices - 1)
            assert list(nrows) == [min(3, depth) + 1, 0, 1, min(2, depth) + 1, 77]
            assert ll[4] == 7.5 and ess[4] == -7
            np.testing.assert_array_equal(ll[:4], wl[:4]); np.testing.assert_array_equal(ess[:4], we[:4])
            _, ref, _ = fl.interpolate([prefix(d, m + 1) for d in datas])
            for a in m6:
                assert np.all(a[1] == 7.5) and np.all(a[4] == 7.5)     # no rows asked for; inactive: the sentinel stays
            for k in (0, 2, 3):
                assert_tail(m6, k, int(nrows[k]), ref[k], exact=True)
        # every series at CSSM_FLEET_NO_ROWS: cssm_fleet_step's bits from one launch
        t = np.array([float(d[0][-1]) + 1.0 for d in datas]); y = np.arange(S, dtype=np.float64)
        ll, ess, nrows, rows, rc = fl.step_interpolate(t, y, lag=[NO] * S, max_lag=2)
        wl, we, wrc = twin.step(t, y)
        np.testing.assert_array_equal(ll, wl); np.testing.assert_array_equal(ess, we); np.testing.assert_array_equal(rc, wrc)
        assert not nrows.any() and all(np.all(np.isnan(a)) for a in rows)
        assert fl.step_interpolate_last_ms()[1] == 0.0
        for k in range(S):
            np.testing.assert_array_equal(fl.particles(k), twin.particles(k))
        # a lag above max_lag names its series
        with pytest.raises(CssmError) as e:
            fl.step_interpolate(t + 1, y, lag=[0, 0, 3, 0, 0], max_lag=2)
        assert e.value.code == _abi.CSSM_EINVAL_ARG and "lag[2] = 3" in str(e.value)


# 6 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [100, 1000])
def test_one_series_fails_and_the_others_do_not_notice(n):
    model = cases.linear_model()
    S, slices = 4, 4
    seeds = [SEED + 17 * k for k in range(S)]
    clean = [cases.gaussian_series(8, seed=SEED + k) for k in range(S)]
    bad = clean[2][1].copy(); bad[3] = 1e200
    datas = list(clean); datas[2] = (clean[2][0], bad, clean[2][2])
    with pytest.raises(oracle.OracleError):                    # the premise: the oracle cannot interpolate that series either
        oracle_interpolate(model, n, seeds[2], datas[2])
    with NativePfFleet(model, n, S) as fl, NativePfFleet(model, n, S) as twin:
        for f in (fl, twin):
            f.reseed(seeds); f.window(slices); f.init([0.0] * S)
        for m in range(8):
            got = fl.step_interpolate(*record(datas, m)[:3], max_lag=3)
            want = twin.step_interpolate(*record(clean, m)[:3], max_lag=3)
            ll, ess, nrows, rows, rc = got
            assert list(rc) == [0, 0, 0 if m < 3 else (_abi.CSSM_ENONFINITE if m == 3 else _abi.CSSM_ESTATE), 0]
            if m >= 3:                                          # its entries are not written, its window is gone
                assert np.isnan(ll[2]) and ess[2] == -1 and nrows[2] == 0 and all(np.all(np.isnan(a[2])) for a in rows)
                assert fl.window_depth(2) == 0
            for k in (0, 1, 3) if m >= 3 else range(S):
                assert ll[k] == want[0][k] and ess[k] == want[1][k] and nrows[k] == want[2][k]
                for a, b in zip(rows, want[3]):
                    np.testing.assert_array_equal(a[k], b[k])
                assert fl.window_depth(k) == min(m + 1, slices - 1)
        fl.init([0.0] * S)                                      # init brings it back, with a fresh window
        assert [fl.window_depth(k) for k in range(S)] == [0] * S
        stream_and_check(fl, [model] * S, seeds, clean, slices, lambda m: 3, 3, calls=5)


# 7 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["linear", "negbin"])
def test_other_observation_models(name):
    S, n, T, slices = 5, 1000, 12, 6
    if name == "linear":
        model, gen = cases.linear_model(), cases.gaussian_series
    else:
        model, gen = cases.literal_case("negbin", T)[0], cases.poisson_counts
    seeds = [SEED + 17 * k for k in range(S)]
    datas = [with_gap(gen(T, seed=SEED + k), T // 3, T // 3 + max(2, T // 5)) for k in range(S)]
    with NativePfFleet(model, n, S) as fl:
        fl.reseed(seeds)
        fl.window(slices)
        fl.init([0.0] * S)
        stream_and_check(fl, [model] * S, seeds, datas, slices, lambda m: 5, 5)


# 8 ------------------------------------------------------------------------------------------------------------------------------
def test_filter_fleet_in_the_reference_vocabulary():
    S, n, T, slices = 3, 500, 9, 4
    models, _, _ = ragged_c2(S)
    datas = []
    for k in range(S):
        t, y, has = with_gap(cases.poisson_counts(T, seed=SEED + k, missing=0.2), 2, 4)
        datas.append([Data(float(a), float(b) if h else None) for a, b, h in zip(t, y, has)])
    lags = [3, None, 1]
    with FilterFleet(models, Resampling.systematicResampling, n, seed=SEED) as ff:
        ff.window(slices)
        states = ff.initialiseState([0.0] * S)
        seen = [[] for _ in range(S)]
        for m in range(T):
            ys = [None if (k == 2 and m == 4) else datas[k][m] for k in range(S)]      # sensor 2 has no datum at call 4
            states, outs = ff.stepInterpolate(states, ys, lags)
            for k in range(S):
                if ys[k] is not None:
                    seen[k].append(ys[k])
            whole = ff.interpolate(seen)                      # (the states stay valid: the fleet is only lent)
            assert len(outs) == S and outs[1] == [] and (m != 4 or outs[2] == [])
            for k in range(S):
                if ys[k] is None or lags[k] is None:
                    assert outs[k] == []
                    continue
                want = whole[k][1][-len(outs[k]):]
                assert len(outs[k]) == min(lags[k], min(len(seen[k]), slices - 1)) + 1
                assert [o.time for o in outs[k]] == sorted(o.time for o in outs[k])     # chronological, oldest first
                for a, b in zip(outs[k], want):
                    assert (a.time, a.observation, a.eta, a.etaIntervals, a.stateIntervals) == (b.time, b.observation, b.eta, b.etaIntervals,
                                                                                                b.stateIntervals)
                    np.testing.assert_array_equal(a.state, b.state)
                    assert formats.pfout_csv(a) == formats.pfout_csv(b)
