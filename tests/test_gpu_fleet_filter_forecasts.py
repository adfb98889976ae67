"""-m gpu: one-step-ahead forecasts of a whole fleet from the launch that filters it (include/cssm_pf.h: cssm_fleet_filter_forecasts,
cssm_fleet_step_forecast; csrc/cssm_fleet_onestep.hip.h) -- ParticleFilter.getMeanForecast mapped over the filter stream
(model/ParticleFilter.scala:368-409) of every series: before a record is weighed, the forecast of its time from the cloud before it.

The reference of every case is the LOOP the call replaces, on a second fleet driven through the entry points that existed before it:
init(t0); per record index forecast([[t_r]] for the series that have one, their keys, want_samples=True), then step(..., active).  Order
statistics AND means are compared with assert_array_equal (the block adds a row in k_fleet_forecast's order, and both launches run blocks
of the fleet's one size); the PIT counts are counted with numpy from the loop's obs sample row; ll, ll_t, ess_t, the final particles,
ancestors and observation index with ==.  In case 1 the first and the last row of every series are also held to the oracle chain plus the
twin draws (expected / check_forecast of tests/test_gpu_forecast.py), so the call does not rest on k_fleet_forecast alone.  No series is
skipped or excused; a status other than zero is asserted where the data provoke it and only there."""
import ctypes as C

import numpy as np
import pytest

import cases
from composablestatespacemodels_amd import Data, _abi
from composablestatespacemodels_amd.filter import FilterFleet, NativePfFleet, Resampling
from composablestatespacemodels_amd.formats import forecast_out_csv
from test_forecast_draws import build_twin
from test_gpu_fleet import run_key
from test_gpu_fleet_interpolate import with_gap
from test_gpu_fleet_intervals import _MODELS, ragged
from test_gpu_forecast import check_forecast, expected

pytestmark = pytest.mark.gpu

SEED = cases.SEED
KEY = 0x0E57E9F0CA57
STAT = NativePfFleet.FORECAST_NAMES
PIT = ("obs_below", "obs_equal")


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    return build_twin(tmp_path_factory.mktemp("twin"))


def record_keys(datas):
    """a Philox key of its own for every record of every series"""
    return [[run_key(KEY + k, r) for r in range(len(d[0]))] for k, d in enumerate(datas)]


def loop(fl, datas, keys, interval, clouds=()):
    """The loop the call replaces, on `fl`: per series a dict of the nine statistics and the two PIT counts ([T_k, ...]; NaN / -1 where
    the loop has no forecast), ll_t, ess_t (NaN / -1 from the record the series failed at), the index of that record (or None), and
    the clouds {(k, r): (particles before record r, clock)} asked for in `clouds`."""
    S, d, n = fl.S, fl.d, fl.n
    T = [len(dd[0]) for dd in datas]
    t0 = np.array([float(np.min(dd[0])) if len(dd[0]) else 0.0 for dd in datas])
    fl.init(t0)
    alive = [Tk > 0 for Tk in T]
    clock = t0.copy()
    out = [{**{name: np.full((T[k], d) if name.startswith("state") else T[k], np.nan) for name in STAT},
            **{name: np.full(T[k], -1, dtype=np.int32) for name in PIT}} for k in range(S)]
    ll_t = [np.full(T[k], np.nan) for k in range(S)]; ess_t = [np.full(T[k], -1, dtype=np.int32) for k in range(S)]
    failed = [None] * S
    seen = {}
    for r in range(max(T)):
        act = np.array([alive[k] and r < T[k] for k in range(S)], dtype=np.uint8)
        if not act.any():
            break
        for (k, rr) in clouds:
            if rr == r and act[k]:
                seen[(k, r)] = (fl.particles(k), float(clock[k]))
        times = [[float(datas[k][0][r])] if act[k] else None for k in range(S)]
        ks = None if keys is None else [keys[k][r] if act[k] else 0 for k in range(S)]
        rs = fl.forecast(times, ks, interval, want_samples=True)
        t = np.array([datas[k][0][r] if act[k] else 0.0 for k in range(S)])
        y = np.array([datas[k][1][r] if act[k] else 0.0 for k in range(S)])
        has = np.array([datas[k][2][r] if act[k] else 0 for k in range(S)], dtype=np.uint8)
        for k in range(S):
            if not act[k] or rs[k]["rc"]:                        # (a time the forecast refuses: the row stays NaN)
                continue
            for name in STAT:
                out[k][name][r] = rs[k][name][0]
            if has[k]:
                obs = rs[k]["samples"][0, d + 2]
                out[k]["obs_below"][r] = int((obs < y[k]).sum()); out[k]["obs_equal"][r] = int((obs == y[k]).sum())
        ll, ess, rc = fl.step(t, y, has, act)
        for k in range(S):
            if not act[k]:
                continue
            if rc[k]:
                assert rc[k] == _abi.CSSM_ENONFINITE, (k, r, rc[k])
                alive[k] = False; failed[k] = r
                continue
            ll_t[k][r] = ll[k]; ess_t[k][r] = ess[k]; clock[k] = t[k]
    return out, ll_t, ess_t, failed, seen


def assert_same_forecasts(got, want, tag):
    for name in STAT + PIT:
        np.testing.assert_array_equal(got[name], want[name], err_msg=f"{tag} {name}")


def nan_rows(fc):
    """the rows of one series without a forecast"""
    return [i for i in range(len(fc["obs_mean"])) if np.isnan(fc["obs_mean"][i])]


def assert_nan_row_is_all_nan(fc, rows, tag):
    for i in rows:
        assert all(np.isnan(fc[name][i]).all() for name in STAT) and all(fc[name][i] == -1 for name in PIT), (tag, i)


# 1 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 63, 100, 1000, _abi.FLEET_MAX_N])
@pytest.mark.parametrize("name", list(_MODELS))
def test_every_row_of_a_ragged_fleet_equals_the_loop(name, n, twin):
    """clamped ranks (1), one pair (2), an odd sub-wave cloud (63), padding to a power of two (100, 1000), the LDS maximum (4096)"""
    make, gen, _ = _MODELS[name]
    model = make()
    datas = ragged(gen)
    S = len(datas)
    seeds = [SEED + 17 * k for k in range(S)]
    keys = record_keys(datas)
    T = [len(d[0]) for d in datas]
    ends = [(k, r) for k in range(S) if T[k] for r in {0, T[k] - 1}]
    with NativePfFleet(model, n, S) as fl, NativePfFleet(model, n, S) as ref:
        fl.reseed(seeds); ref.reseed(seeds)
        for interval, ky in ((0.975, keys), (0.5, keys), (1.0, keys), (0.975, None)):
            ll, ll_t, ess_t, fc, rc, fc_rc = fl.filter_forecasts(datas, interval, ky)
            want, wll_t, wess_t, failed, clouds = loop(ref, datas, ky, interval, ends if ky is keys and interval == 0.975 else ())
            assert list(rc) == [0, _abi.CSSM_EINVAL_ARG, 0, _abi.CSSM_ENONFINITE, 0], rc
            assert not fc_rc.any(), fc_rc
            assert failed == [None, None, None, 2, None], "the premise: the loop cannot move series 3 backwards in time either"
            # where the NaN rows are: none; nothing written; none; the refused time and everything behind the failure; none
            assert [nan_rows(fc[k]) for k in range(S)] == [[], [], [], [2, 3], []]
            for k in range(S):
                tag = (name, n, interval, ky is None, k)
                assert all(len(fc[k][nm]) == T[k] for nm in STAT + PIT)
                assert_same_forecasts(fc[k], want[k], tag)
                assert_nan_row_is_all_nan(fc[k], nan_rows(fc[k]), tag)
                np.testing.assert_array_equal(ll_t[k], wll_t[k]); np.testing.assert_array_equal(ess_t[k], wess_t[k])
                has = np.asarray(datas[k][2], dtype=bool)
                ok = ~np.isnan(fc[k]["obs_mean"])
                assert np.all((fc[k]["obs_below"] >= 0) == (has & ok)) and np.all((fc[k]["obs_equal"] >= 0) == (has & ok)), tag
                assert np.all(fc[k]["obs_below"][has & ok] + fc[k]["obs_equal"][has & ok] <= n)
                if T[k] == 0 or failed[k] is not None:
                    assert np.isnan(ll[k])
                    continue
                assert ll[k] == wll_t[k][-1]
                np.testing.assert_array_equal(fl.particles(k), ref.particles(k))
                np.testing.assert_array_equal(fl.ancestors(k), ref.ancestors(k))
                assert fl.observation_index(k) == ref.observation_index(k) == T[k]
            for (k, r), (cloud, clock) in clouds.items():        # ... and the oracle chain + twin draws from the cloud before the record
                exp = expected(model, cloud, clock, np.array([datas[k][0][r]]), keys[k][r], twin)
                row = {nm: fc[k][nm][r:r + 1] for nm in STAT}
                row["samples"] = None
                check_forecast(row, *exp, interval=interval)
                if datas[k][2][r]:
                    y = datas[k][1][r]
                    assert (fc[k]["obs_below"][r], fc[k]["obs_equal"][r]) == (int((exp[2][0] < y).sum()), int((exp[2][0] == y).sum()))
            if ky is keys and interval == 0.975:
                assert sorted(clouds) == sorted(e for e in ends if e != (3, 3)), "every first and last row but the dead series' last"


def assert_whole_fleet_equals_the_loop(fl, ref, models, datas, keys, interval, rows, twin):
    """`filter_forecasts(datas, interval, keys)` on `fl` of a fleet no series of which fails, against loop() on `ref` (the same models and
    seeds): every row of every series, ll_t, ess_t, ll and the clouds both fleets hold afterwards; and rows[k] (record indices) of series
    k against the oracle chain + twin draws from the cloud before the record, PIT counts included -- k_fleet_forecast, which the loop
    runs, is one body with the kernel under test."""
    S, n = fl.S, fl.n
    T = [len(d[0]) for d in datas]
    asked = [(k, r) for k in range(S) for r in rows[k]]
    ll, ll_t, ess_t, fc, rc, fc_rc = fl.filter_forecasts(datas, interval, keys)
    want, wll_t, wess_t, failed, clouds = loop(ref, datas, keys, interval, asked)
    assert not rc.any() and not fc_rc.any() and failed == [None] * S, (rc, fc_rc, failed)
    for k in range(S):
        assert all(len(fc[k][nm]) == T[k] for nm in STAT + PIT)
        assert_same_forecasts(fc[k], want[k], (n, interval, k))
        assert nan_rows(fc[k]) == []
        np.testing.assert_array_equal(ll_t[k], wll_t[k]); np.testing.assert_array_equal(ess_t[k], wess_t[k])
        has = np.asarray(datas[k][2], dtype=bool)
        assert np.all((fc[k]["obs_below"] >= 0) == has) and np.all((fc[k]["obs_equal"] >= 0) == has), (n, k)
        assert ll[k] == wll_t[k][-1]
        np.testing.assert_array_equal(fl.particles(k), ref.particles(k))
        np.testing.assert_array_equal(fl.ancestors(k), ref.ancestors(k))
        assert fl.observation_index(k) == ref.observation_index(k) == T[k]
    assert sorted(clouds) == sorted(asked)
    for (k, r), (cloud, clock) in clouds.items():
        exp = expected(models[k], cloud, clock, np.array([datas[k][0][r]]), keys[k][r], twin)
        row = {nm: fc[k][nm][r:r + 1] for nm in STAT}
        row["samples"] = None
        check_forecast(row, *exp, interval=interval)
        y = datas[k][1][r]
        pit = (int((exp[2][0] < y).sum()), int((exp[2][0] == y).sum())) if datas[k][2][r] else (-1, -1)
        assert (fc[k]["obs_below"][r], fc[k]["obs_equal"][r]) == pit, (n, k, r)


@pytest.mark.parametrize("d", list(range(1, 17)))
def test_every_latent_dimension(d, twin):
    """k_fleet_series<d, FCST> from both entry points on the per-dimension fixture of the sibling files: every row against the loop; rows
    0, 4 (the first record behind the gap: the cloud before it is read through identity ancestors) and 5 (the last) against the oracle
    chain; then one streamed record (one series without a datum) against forecast + step."""
    model = cases.dim_model(d)
    S, n = 3, 257
    seeds = [SEED + 17 * k for k in range(S)]
    datas = [with_gap(cases.poisson_counts(6, seed=SEED + k), 2, 4) for k in range(S)]
    keys = record_keys(datas)
    with NativePfFleet(model, n, S) as fl, NativePfFleet(model, n, S) as ref:
        assert fl.d == ref.d == d
        fl.reseed(seeds); ref.reseed(seeds)
        assert_whole_fleet_equals_the_loop(fl, ref, [model] * S, datas, keys, 0.975, [(0, 4, 5)] * S, twin)
        t = np.array([float(dd[0][-1]) + 0.75 for dd in datas]); y = np.array([1.0, 3.0, 0.0])
        has = np.array([1, 0, 1], dtype=np.uint8); active = np.ones(S, dtype=np.uint8)
        ky = np.array([run_key(KEY + 99, k) for k in range(S)], dtype=np.uint64)
        ll, ess, arr, rc, fc_rc = _raw_step_forecast(fl, t, y, has, active, ky, 0.5, 7.5)
        rs = ref.forecast([[v] for v in t], [int(v) for v in ky], 0.5, want_samples=True)
        lb, eb, rb = ref.step(t, y, has, active)
        assert not rc.any() and not rb.any() and not fc_rc.any(), (rc, rb, fc_rc)
        for k in range(S):
            assert ll[k] == lb[k] and ess[k] == eb[k] and rs[k]["rc"] == 0, (d, k)
            for nm in STAT:
                np.testing.assert_array_equal(arr[nm][k], rs[k][nm][0], err_msg=f"d {d} series {k} {nm}")
            obs = rs[k]["samples"][0, d + 2]
            pit = (int((obs < y[k]).sum()), int((obs == y[k]).sum())) if has[k] else (-1, -1)
            assert (arr["obs_below"][k], arr["obs_equal"][k]) == pit, (d, k)
            np.testing.assert_array_equal(fl.particles(k), ref.particles(k))
            np.testing.assert_array_equal(fl.ancestors(k), ref.ancestors(k))


# 2 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [100, 1000])
def test_a_series_that_fails_mid_way_keeps_its_rows_and_nobody_notices(n):
    """series 2's observation 3 is an outlier no particle can be weighed against: its forecast rows 0 .. 3 are the loop's (row 3 is formed
    before the weighing), rows 4 .. are NaN, and the neighbours are bit for bit the same fleet without it"""
    model = cases.linear_model()
    S = 4
    seeds = [SEED + 17 * k for k in range(S)]
    datas = [cases.gaussian_series(6 + k, seed=SEED + k) for k in range(S)]
    bad = datas[2][1].copy(); bad[3] = 1e200
    datas[2] = (datas[2][0], bad, datas[2][2])
    keys = record_keys(datas)
    keep = [0, 1, 3]
    with NativePfFleet(model, n, S) as fl, NativePfFleet(model, n, 3) as f3, NativePfFleet(model, n, S) as ref:
        fl.reseed(seeds); f3.reseed([seeds[k] for k in keep]); ref.reseed(seeds)
        ll, ll_t, ess_t, fc, rc, fc_rc = fl.filter_forecasts(datas, 0.9, keys)
        ll3, ll_t3, ess_t3, fc3, rc3, fc_rc3 = f3.filter_forecasts([datas[k] for k in keep], 0.9, [keys[k] for k in keep])
        want, wll_t, wess_t, failed, _ = loop(ref, datas, keys, 0.9)
        assert list(rc) == [0, 0, _abi.CSSM_ENONFINITE, 0] and not rc3.any() and not fc_rc.any() and not fc_rc3.any()
        assert failed == [None, None, 3, None]                   # (the premise: the loop cannot weigh that observation either)
        for j, k in enumerate(keep):
            assert ll[k] == ll3[j]
            np.testing.assert_array_equal(ll_t[k], ll_t3[j]); np.testing.assert_array_equal(ess_t[k], ess_t3[j])
            assert_same_forecasts(fc[k], fc3[j], (n, k, "without the failing series"))
            np.testing.assert_array_equal(fl.particles(k), f3.particles(j))
        for k in range(S):
            assert_same_forecasts(fc[k], want[k], (n, k))
            np.testing.assert_array_equal(ll_t[k], wll_t[k]); np.testing.assert_array_equal(ess_t[k], wess_t[k])
        assert nan_rows(fc[2]) == [4, 5, 6, 7] and [nan_rows(fc[k]) for k in keep] == [[], [], []]
        assert fc[2]["obs_below"][3] >= 0 and np.isfinite(fc[2]["obs_mean"][3])
        assert_nan_row_is_all_nan(fc[2], [4, 5, 6, 7], n)
        assert np.isnan(ll[2]) and np.isnan(ll_t[2][3:]).all()


# 3 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [100, 1000])
def test_the_fleet_afterwards_is_the_one_ll_filter_leaves(n):
    model = cases.c2_model()
    datas = [d for k, d in enumerate(ragged(cases.poisson_counts)) if k in (0, 2, 4)]
    S = len(datas)
    seeds = [SEED + 17 * k for k in range(S)]
    with NativePfFleet(model, n, S) as fa, NativePfFleet(model, n, S) as fb:
        fa.reseed(seeds); fb.reseed(seeds)
        ll, ll_t, ess_t, fc, rc, fc_rc = fa.filter_forecasts(datas, 0.8, record_keys(datas))
        assert fa.last_ms()[0] > 0.0
        llb, ll_tb, ess_tb, rcb = fb.ll_filter(datas)
        assert not rc.any() and not rcb.any() and not fc_rc.any()
        np.testing.assert_array_equal(ll, llb)
        for k in range(S):
            np.testing.assert_array_equal(ll_t[k], ll_tb[k]); np.testing.assert_array_equal(ess_t[k], ess_tb[k])
            np.testing.assert_array_equal(fa.particles(k), fb.particles(k))
            np.testing.assert_array_equal(fa.ancestors(k), fb.ancestors(k))
            assert fa.observation_index(k) == fb.observation_index(k) == len(datas[k][0])
        for a, b in zip(fa.summary(0.8), fb.summary(0.8)):
            np.testing.assert_array_equal(a, b)
        times = [[d[0][-1] + 0.25, d[0][-1] + 0.25, d[0][-1] + 2.0] for d in datas]
        for ra, rb in zip(fa.forecast(times, None, 0.9, want_samples=True), fb.forecast(times, None, 0.9, want_samples=True)):
            assert ra["rc"] == rb["rc"] == 0 and ra["key"] == rb["key"]
            for name in STAT + ("samples",):
                np.testing.assert_array_equal(ra[name], rb[name], err_msg=name)
        t = np.array([d[0][-1] + 0.75 for d in datas]); y = np.array([1.0, 3.0, 0.0])
        la, ea, ra = fa.step(t, y)
        lb, eb, rb = fb.step(t, y)
        assert not ra.any() and not rb.any()
        np.testing.assert_array_equal(la, lb); np.testing.assert_array_equal(ea, eb)
        for k in range(S):
            np.testing.assert_array_equal(fa.particles(k), fb.particles(k))
            np.testing.assert_array_equal(fa.ancestors(k), fb.ancestors(k))


# 4 ------------------------------------------------------------------------------------------------------------------------------
def _raw_step_forecast(fl, t, y, has, active, keys, interval, sentinel):
    """cssm_fleet_step_forecast through the C ABI with every output preset to a sentinel of the test's own"""
    S, d = fl.S, fl.d
    p = lambda a, ty=C.c_double: a.ctypes.data_as(C.POINTER(ty))
    ll = np.full(S, sentinel); ess = np.full(S, -77, dtype=np.int32); rc = np.full(S, -77, dtype=np.int32); fc_rc = np.full(S, -77, dtype=np.int32)
    arr = {name: np.full((S, d) if name.startswith("state") else S, sentinel) for name in STAT}
    arr.update({name: np.full(S, -77, dtype=np.int32) for name in PIT})
    assert fl.lib.cssm_fleet_step_forecast(fl._h, p(active, C.c_uint8), p(t), p(y), p(has, C.c_uint8), p(keys, C.c_uint64), interval, p(ll),
                                           p(ess, C.c_int32), *[p(arr[name]) for name in STAT], *[p(arr[name], C.c_int32) for name in PIT],
                                           p(rc, C.c_int), p(fc_rc, C.c_int)) == 0, fl.lib.cssm_last_error()
    return ll, ess, arr, rc, fc_rc


@pytest.mark.parametrize("name,n", [("c2", 100), ("c2", 1000), ("dim9", 100), ("linear", _abi.FLEET_MAX_N), ("bernoulli", 2)])
def test_streaming_steps_with_forecasts_equal_forecast_then_step(name, n):
    make, gen, _ = _MODELS[name]
    model = make()
    S, rounds = 5, 8
    seeds = [SEED + 17 * k for k in range(S)]
    ys = [gen(rounds, seed=SEED + k)[1] for k in range(S)]
    clock = np.array([0.5 * k for k in range(S)])
    with NativePfFleet(model, n, S) as fa, NativePfFleet(model, n, S) as fb:
        fa.reseed(seeds); fb.reseed(seeds)
        fa.init(clock); fb.init(clock)
        for r in range(rounds):
            interval = (0.975, 0.6, 1.0)[r % 3]
            active = np.array([(r + k) % 3 != 0 for k in range(S)], dtype=np.uint8)
            has = np.array([(r * 5 + k) % 4 != 0 for k in range(S)], dtype=np.uint8)
            clock = clock + np.where(active != 0, 0.25 * ((r + np.arange(S)) % 3), 0.0)      # (dt = 0 among them)
            y = np.array([ys[k][r] for k in range(S)])
            keys = np.array([run_key(KEY + r, k) for k in range(S)], dtype=np.uint64)
            ll, ess, arr, rc, fc_rc = _raw_step_forecast(fa, clock, y, has, active, keys, interval, 7.5)
            rs = fb.forecast([[clock[k]] if active[k] else None for k in range(S)], [int(v) for v in keys], interval, want_samples=True)
            lb, eb, rb = fb.step(clock, y, has, active)
            assert not rc.any() and not rb.any() and not fc_rc.any(), (r, rc, rb, fc_rc)
            for k in range(S):
                if not active[k]:                                # untouched: the sentinels stand
                    assert ll[k] == 7.5 and ess[k] == -77 and all(np.all(arr[nm][k] == 7.5) for nm in STAT), (r, k)
                    assert arr["obs_below"][k] == -77 and arr["obs_equal"][k] == -77, (r, k)
                    continue
                assert ll[k] == lb[k] and ess[k] == eb[k] and rs[k]["rc"] == 0, (r, k)
                for nm in STAT:
                    np.testing.assert_array_equal(arr[nm][k], rs[k][nm][0], err_msg=f"round {r} series {k} {nm}")
                obs = rs[k]["samples"][0, fa.d + 2]
                want = (int((obs < y[k]).sum()), int((obs == y[k]).sum())) if has[k] else (-1, -1)
                assert (arr["obs_below"][k], arr["obs_equal"][k]) == want, (r, k)
        for k in range(S):
            np.testing.assert_array_equal(fa.particles(k), fb.particles(k))
            np.testing.assert_array_equal(fa.ancestors(k), fb.ancestors(k))
            assert fa.observation_index(k) == fb.observation_index(k)
        # the default keys: cssm_pf_run_key(seed_k, 2^63 | observation index), and the Python mirror of the call
        t = clock + 0.5; y = np.array([ys[k][0] for k in range(S)])
        want = fb.forecast([[v] for v in t], None, 0.975, want_samples=True)
        ll, ess, arr, rc, fc_rc = fa.step_forecast(t, y)
        assert not rc.any() and not fc_rc.any()
        for k in range(S):
            for nm in STAT:
                np.testing.assert_array_equal(arr[nm][k], want[k][nm][0], err_msg=nm)
            obs = want[k]["samples"][0, fa.d + 2]
            assert (arr["obs_below"][k], arr["obs_equal"][k]) == (int((obs < y[k]).sum()), int((obs == y[k]).sum()))


# 5 ------------------------------------------------------------------------------------------------------------------------------
def test_more_series_than_the_gpu_holds_blocks_at_once():
    model = cases.c2_model()
    S, n, T = 2048, 100, 3
    seeds = [SEED + 17 * k for k in range(S)]
    base = [cases.poisson_counts(T, seed=SEED + j, dt=(1.0, 0.5, 0.25)[j % 3], missing=0.2) for j in range(16)]
    datas = [(base[k % 16][0] + 0.125 * (k % 5), base[k % 16][1], base[k % 16][2]) for k in range(S)]
    keys = [[run_key(KEY + (k % 64), r) for r in range(T)] for k in range(S)]
    with NativePfFleet(model, n, S) as fl, NativePfFleet(model, n, S) as ref:
        fl.reseed(seeds); ref.reseed(seeds)
        ll, ll_t, ess_t, fc, rc, fc_rc = fl.filter_forecasts(datas, 0.975, keys)
        want, wll_t, wess_t, failed, _ = loop(ref, datas, keys, 0.975)
        assert not rc.any() and not fc_rc.any() and failed == [None] * S
        for k in list(range(0, S, 37)) + [S - 1]:
            assert_same_forecasts(fc[k], want[k], k)
            assert nan_rows(fc[k]) == []
            np.testing.assert_array_equal(ll_t[k], wll_t[k]); np.testing.assert_array_equal(ess_t[k], wess_t[k])
            np.testing.assert_array_equal(fl.particles(k), ref.particles(k))


# 6 ------------------------------------------------------------------------------------------------------------------------------
def test_filter_fleet_writes_the_lines_of_getmeanforecast_then_stepfilter():
    """FilterFleet.filterForecasts: one ForecastOut per datum at the datum's time; their forecast_out_csv lines are those of getMeanForecast
    + stepFilter in a loop, and stepForecast gives the same ForecastOuts a step at a time"""
    um = cases.c2_unparam()
    S, n = 3, 500
    p0 = cases.c2_params()
    th = np.asarray(p0.flattenParams())
    mods = [um.run(p0.withFlat(th + 0.02 * k * np.cos(np.arange(th.size) + k))) for k in range(S)]
    datas = []
    for k in range(S):
        t, y, has = cases.poisson_counts(5 + 3 * k, seed=SEED + k, dt=(1, .5, .25)[k], missing=0.25)
        datas.append([Data(float(a) + k, float(b) if h else None) for a, b, h in zip(t, y, has)])
    t0 = [min(d.t for d in data) for data in datas]
    with FilterFleet(mods, Resampling.systematicResampling, n, seed=SEED) as ff:
        outs = ff.filterForecasts(datas, 0.9)
    assert [len(o) for o in outs] == [len(d) for d in datas]
    for k in range(S):
        assert [o.t for o in outs[k]] == [d.t for d in datas[k]]
    lines = [[forecast_out_csv(o) for o in outs[k]] for k in range(S)]
    with FilterFleet(mods, Resampling.systematicResampling, n, seed=SEED) as ff, FilterFleet(mods, Resampling.systematicResampling, n, seed=SEED) as fs:
        st = ff.initialiseState(t0); ss = fs.initialiseState(t0)
        loop_lines = [[] for _ in range(S)]; stream = [[] for _ in range(S)]
        for r in range(max(len(d) for d in datas)):
            obs = [d[r] if r < len(d) else None for d in datas]
            got = ff.forecast([[o.t] if o is not None else None for o in obs], 0.9)      # (getMeanForecast of the series that have a datum)
            st = ff.stepFilter(st, obs)
            ss, souts = fs.stepForecast(ss, obs, 0.9)
            for k in range(S):
                if obs[k] is not None:
                    loop_lines[k].append(forecast_out_csv(got[k][0]))
                    stream[k].append(forecast_out_csv(souts[k]))
                    assert souts[k].t == obs[k].t
                else:
                    assert souts[k] is None
        one = ff.getMeanForecast([st[k].t + 1.0 for k in range(S)], 0.9)                # (the call the loop stands for, on every series)
        assert len(one) == S
    assert lines == loop_lines
    assert lines == stream


# 7 ------------------------------------------------------------------------------------------------------------------------------
def test_a_model_without_the_scale_its_observation_needs():
    """BetaModel without a shape: the filter runs, the observation cannot be drawn (the reference throws).  Every series' forecast status
    is CSSM_EINVAL_ARG, its forecast rows read NaN / -1, the call succeeds with the reference's exception as its message, and the filter
    results are those of ll_filter."""
    model = cases.beta_model()
    S, n, T = 3, 100, 5
    seeds = [SEED + 17 * k for k in range(S)]
    datas = [cases.unit_interval_series(T + k, seed=SEED + k) for k in range(S)]
    with NativePfFleet(model, n, S) as fa, NativePfFleet(model, n, S) as fb:
        fa.reseed(seeds); fb.reseed(seeds)
        ll, ll_t, ess_t, fc, rc, fc_rc = fa.filter_forecasts(datas, 0.975)
        msg = fa.lib.cssm_last_error()
        assert b"series 0" in msg and b"Must provide shape parameter for Beta Model" in msg
        llb, ll_tb, ess_tb, rcb = fb.ll_filter(datas)
        assert not rc.any() and not rcb.any() and list(fc_rc) == [_abi.CSSM_EINVAL_ARG] * S
        np.testing.assert_array_equal(ll, llb)
        for k in range(S):
            assert nan_rows(fc[k]) == list(range(T + k))
            assert_nan_row_is_all_nan(fc[k], range(T + k), k)
            np.testing.assert_array_equal(ll_t[k], ll_tb[k]); np.testing.assert_array_equal(ess_t[k], ess_tb[k])
            np.testing.assert_array_equal(fa.particles(k), fb.particles(k))
            np.testing.assert_array_equal(fa.ancestors(k), fb.ancestors(k))
        t = np.array([d[0][-1] + 0.5 for d in datas]); y = np.full(S, 0.5)
        la, ea, arr, ra, fra = fa.step_forecast(t, y)
        lb, eb, rb = fb.step(t, y)
        assert not ra.any() and not rb.any() and list(fra) == [_abi.CSSM_EINVAL_ARG] * S
        np.testing.assert_array_equal(la, lb); np.testing.assert_array_equal(ea, eb)
        assert all(np.isnan(arr[nm]).all() for nm in STAT) and all((arr[nm] == -1).all() for nm in PIT)
