"""GPU tests of the LGCP fleet (include/cssm_pf.h: cssm_fleet_create_lgcp): many Cox-process event streams filtered per launch, every
series bit for bit the oracle's FilterLgcp and a handle's of its own.  Every comparison is == / assert_array_equal unless it says
otherwise; no series is skipped."""
import ctypes as C

import numpy as np
import pytest

import cases
from composablestatespacemodels_amd import _abi
from composablestatespacemodels_amd.filter import FilterFleet, FilterLgcp, FilterLgcpFleet, NativeLgcpFleet, NativePf, Resampling
from composablestatespacemodels_amd.model import Model, Parameters, Sde, SdeParameter
from composablestatespacemodels_amd.simulate import lgcp_events_data, lgcp_fleet_data, simulate_lgcp
from oracle import oracle

pytestmark = pytest.mark.gpu

SEED = cases.SEED
# the level fixture: a first event at t0 (dt = 0, no prediction), a repeated time in mid-stream, a gap of 40 (the max falls by more than
# the prediction tolerates), a short step behind it (the max rises back by more than the margin)
FIXTURE = np.array([0.0, 0.05, 0.05, 0.3, 0.31, 40.31, 40.4, 40.45])


def c4_params():
    return Parameters.apply(None, SdeParameter.ouParameter(0.1, 0.5, 0.4, 0.1, 0.5))


def _perturbed(make_params, k):
    """series k's parameters: the model's own, shifted a little per series (the structures stay equal)"""
    p = make_params()
    th = np.asarray(p.flattenParams())
    return p.withFlat(th + 0.03 * (k % 7) * np.cos(np.arange(th.size) + k))


def events(t):
    t = np.ascontiguousarray(t, dtype=np.float64)
    return t, np.ones(len(t)), np.ones(len(t), dtype=np.uint8)


_ORACLE = {}


def oracle_run(key, model, precision, n, seed, t):
    """the oracle's llFilter of one stream, computed once per (key, n, seed): (ll, ll_t, ess_t, particles, ancestors, summary)"""
    k = (key, precision, n, seed, tuple(np.asarray(t).tolist()))
    if k not in _ORACLE:
        o = oracle.OraclePf(model.descriptor(precision), n, seed)
        ll, ll_t, ess_t, _ = o.filter(*events(t))
        for a in (ll_t, ess_t):
            a.setflags(write=False)
        _ORACLE[k] = (ll, ll_t, ess_t, o.particles(), o.ancestors(), o.summary(0.975))
    return _ORACLE[k]


def oracle_runs(jobs):
    """``oracle_run`` of several streams side by side (the oracle's handles are independent and its calls leave the interpreter)"""
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=8) as ex:
        return list(ex.map(lambda j: oracle_run(*j), jobs))


def assert_series_is_the_oracle(fl, k, want, ll, ll_t, ess_t):
    oll, oll_t, oess_t, ox, oa, _ = want
    assert ll[k] == oll, (k, ll[k], oll)
    np.testing.assert_array_equal(ll_t[k], oll_t)
    np.testing.assert_array_equal(ess_t[k], oess_t)
    np.testing.assert_array_equal(fl.particles(k), ox)
    np.testing.assert_array_equal(fl.ancestors(k), oa)


def assert_series_is_a_handle(fl, k, model, precision, n, seed, t, ll, ll_t, ess_t):
    with NativePf(model, n, seed, lgcp_precision=precision) as g:
        gl, gll_t, gess_t, _ = g.run(*events(t))
        assert ll[k] == gl, (k, ll[k], gl)
        np.testing.assert_array_equal(ll_t[k], gll_t)
        np.testing.assert_array_equal(ess_t[k], gess_t)
        np.testing.assert_array_equal(fl.particles(k), g.particles())
        np.testing.assert_array_equal(fl.ancestors(k), g.ancestors())


# 1 ------------------------------------------------------------------------------------------------------------------------------
def level_branches(n):
    """per record of the fixture on the oracle: (the predicted level c, the level used, the max)"""
    o = oracle.OraclePf(cases.c4_model().descriptor(2), n, SEED)
    o.init(float(FIXTURE[0]))
    out = []
    for t in FIXTURE:
        c = o.ref_level(1.0)                       # (LGCP: the level predicted from the event before; NaN while there is none)
        o.step(float(t), 1.0, True)
        out.append((c,) + o.ref())
    return out


@pytest.mark.parametrize("n", [63, 1000])
def test_the_level_fixture_takes_every_branch(n):
    """a condition on the fixture, not a tolerance: the prediction is absent (record 0), kept (1, 3, 4, 7), ruled out because the max
    fell by more than 24 (record 5) and ruled out because it rose by more than 8 (record 6); records 0 and 2 have dt = 0"""
    br = level_branches(n)
    assert FIXTURE[0] == 0.0 and FIXTURE[2] == FIXTURE[1]
    assert np.isnan(br[0][0]) and br[0][1] == br[0][2]
    for s in (1, 3, 4, 7):
        c, ref, gmax = br[s]
        assert ref == c and c != gmax, (s, br[s])
    for s in (2,):                                  # (dt = 0 in mid-stream: every weight is gamma - gamma = 0, the max is 0)
        assert br[s][2] == 0.0
    c, ref, gmax = br[5]
    assert ref == gmax and c - gmax > 32.0 and br[4][2] - gmax > 24.0, br[5]
    c, ref, gmax = br[6]
    assert ref == gmax and c - gmax < 0.0 and gmax - br[5][2] > 8.0, br[6]
    for s in range(1, 8):                           # the chain itself: every prediction is the max before plus the margin
        assert br[s][0] == br[s - 1][2] + 8.0


@pytest.mark.parametrize("n", [1, 2, 63, 100, 1000, _abi.FLEET_MAX_N])
def test_level_fixture_fleet_equals_the_oracle_and_handles_of_its_own(n):
    S, model = 6, cases.c4_model()
    seeds = [SEED + 17 * k for k in range(S)]
    datas = [FIXTURE + 3.0 * k for k in range(S)]
    want = oracle_runs([("fixture", model, 2, n, seeds[k], datas[k]) for k in range(S)])
    with NativeLgcpFleet(model, n, S, 2) as fl:
        fl.reseed(seeds)
        ll, ll_t, ess_t, rc = fl.ll_filter(datas)
        assert not rc.any(), rc
        for k in range(S):
            assert_series_is_the_oracle(fl, k, want[k], ll, ll_t, ess_t)
            assert fl.observation_index(k) == len(FIXTURE)
            if n in (100, _abi.FLEET_MAX_N):
                assert_series_is_a_handle(fl, k, model, 2, n, seeds[k], datas[k], ll, ll_t, ess_t)


# 2, 8 ---------------------------------------------------------------------------------------------------------------------------
def ragged_c4(S=12):
    um = Model.lgcp(Sde.ouProcess(1))
    models = [um.run(_perturbed(c4_params, k)) for k in range(S)]
    seeds = [SEED + 17 * k for k in range(S)]
    datas = [cases.event_times(3 + (5 * k) % 11, seed=SEED + k, horizon=2.0)[0] for k in range(S)]
    return models, seeds, datas


@pytest.mark.parametrize("n", [257, 1000])
def test_ragged_streams_twice_and_their_summary(n):
    S = 12
    models, seeds, datas = ragged_c4(S)
    with NativeLgcpFleet(models[0], n, S, 2) as fl:
        fl.set_params(models)
        for sd in (seeds, seeds[1:] + seeds[:1]):           # the same fleet again with the seeds rotated by one (buffers reused)
            fl.reseed(sd)
            ll, ll_t, ess_t, rc = fl.ll_filter(datas)
            assert not rc.any(), rc
            got = fl.summary(0.975)
            for k in range(S):
                want = oracle_run(("ragged", k), models[k], 2, n, sd[k], datas[k])
                assert_series_is_the_oracle(fl, k, want, ll, ll_t, ess_t)
                # test_gpu_fleet.py's rules: order statistics bit for bit, the means (plain fp64 sums in another order) within rtol 1e-12
                m, lo, hi, em, el, eu = got
                om, olo, ohi, oem, oel, oeu = want[5]
                np.testing.assert_array_equal(lo[k], olo)
                np.testing.assert_array_equal(hi[k], ohi)
                assert el[k] == oel and eu[k] == oeu
                np.testing.assert_allclose(m[k], om, rtol=1e-12, atol=0)
                np.testing.assert_allclose(em[k], oem, rtol=1e-12, atol=0)


# 3 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 2, 3, 4, 5, 8, 9, 16])
def test_latent_dimension_and_box_muller_parity(d):
    """d odd: the parity of a sub-step's first normal alternates, a Box-Muller pair and a Philox block straddle sub-steps"""
    p = Parameters.apply(None, SdeParameter.ouParameter(0.1, 0.5, 0.4, [0.1 + 0.05 * c for c in range(d)], 0.5))
    model = Model.lgcp(Sde.ouProcess(d)).run(p)
    S, n = 3, 130
    seeds = [SEED + 17 * k for k in range(S)]
    datas = [np.cumsum([0.25, 0.4, 0.55, 0.7, 0.3]) + 1.5 * k for k in range(S)]
    with NativeLgcpFleet(model, n, S, 1) as fl:
        fl.reseed(seeds)
        ll, ll_t, ess_t, rc = fl.ll_filter(datas)
        assert not rc.any(), rc
        for k in range(S):
            assert_series_is_the_oracle(fl, k, oracle_run(("dim", d), model, 1, n, seeds[k], datas[k]), ll, ll_t, ess_t)


# 4 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [257, 1000])
def test_time_dependent_f(n):
    model = cases.lgcp_seasonal_model()
    S = 5
    seeds = [SEED + 17 * k for k in range(S)]
    datas = [cases.event_times(6, seed=SEED + 40 + k, horizon=3.0)[0] + 7.25 * k for k in range(S)]
    with NativeLgcpFleet(model, n, S, 1) as fl:
        fl.reseed(seeds)
        ll, ll_t, ess_t, rc = fl.ll_filter(datas)
        assert not rc.any(), rc
        for k in range(S):
            assert_series_is_the_oracle(fl, k, oracle_run("seasonal", model, 1, n, seeds[k], datas[k]), ll, ll_t, ess_t)
            if n == 257:
                assert_series_is_a_handle(fl, k, model, 1, n, seeds[k], datas[k], ll, ll_t, ess_t)


# 5 ------------------------------------------------------------------------------------------------------------------------------
def stream(fl, datas, t0s, third_out=True, check=None):
    """init, then one step per event index; every other call leaves a third of the series out (they catch up in a call of their own)"""
    S = fl.S
    fl.init(t0s)
    ll, ess = np.zeros(S), np.zeros(S, dtype=np.int32)
    T = max(len(d) for d in datas)
    for s in range(T):
        has = np.array([1 if s < len(d) else 0 for d in datas], dtype=np.uint8)
        t = np.array([d[s] if s < len(d) else 0.0 for d in datas])
        groups = [has.copy()]
        if third_out and s % 2 == 1:
            out = np.array([1 if k % 3 == 1 else 0 for k in range(S)], dtype=np.uint8)
            groups = [has & (1 - out), has & out]
        for act in groups:
            if not act.any():
                continue
            l, e, rc = fl.step(t, np.ones(S), None, act)
            assert not rc.any(), rc
            ll[act == 1] = l[act == 1]; ess[act == 1] = e[act == 1]
        if check is not None:
            check(s)
    return ll, ess


def test_streaming_is_ll_filter_bit_for_bit():
    S, n, model = 6, 300, cases.c4_model()
    seeds = [SEED + 17 * k for k in range(S)]
    datas = [FIXTURE[:7] + 3.0 * k if k % 2 == 0 else cases.event_times(5 + k, seed=SEED + k, horizon=2.0)[0] for k in range(S)]
    t0s = np.array([d[0] for d in datas])
    with NativeLgcpFleet(model, n, S, 2) as fresh, NativeLgcpFleet(model, n, S, 2) as fl:
        fresh.reseed(seeds); fl.reseed(seeds)
        ll, ll_t, ess_t, rc = fresh.ll_filter(datas)
        assert not rc.any(), rc

        def middle(s):                              # after event 2 of every stream: the oracle stepped to the same event
            if s != 2:
                return
            for k in range(S):
                o = oracle.OraclePf(model.descriptor(2), n, seeds[k])
                o.init(float(t0s[k]))
                for q in range(3):
                    o.step(float(datas[k][q]), 1.0, True)
                np.testing.assert_array_equal(fl.particles(k), o.particles())
                np.testing.assert_array_equal(fl.ancestors(k), o.ancestors())
        sl, se = stream(fl, datas, t0s, check=middle)
        for k in range(S):
            assert sl[k] == ll[k] and se[k] == ess_t[k][-1], k
            np.testing.assert_array_equal(fl.particles(k), fresh.particles(k))
            np.testing.assert_array_equal(fl.ancestors(k), fresh.ancestors(k))
        # a new cloud forgets the level: another t0, a second stream, against a fleet that never ran the first
        datas2 = [d + 11.0 for d in datas[::-1]]
        t02 = np.array([d[0] - 0.5 for d in datas2])
        sl2, se2 = stream(fl, datas2, t02)
        with NativeLgcpFleet(model, n, S, 2) as other:
            other.reseed(seeds)
            ol2, oe2 = stream(other, datas2, t02, third_out=False)
            for k in range(S):
                assert sl2[k] == ol2[k] and se2[k] == oe2[k], k
                np.testing.assert_array_equal(fl.particles(k), other.particles(k))
        # ll_filter of a prefix, then step: the stream goes on bit for bit (the level crosses the launches)
        head = [d[:4] for d in datas]
        _, _, _, rc = fl.ll_filter(head)
        assert not rc.any(), rc
        T = max(len(d) for d in datas)
        last = np.zeros(S)
        for s in range(4, T):
            act = np.array([1 if s < len(d) else 0 for d in datas], dtype=np.uint8)
            l, _, rc = fl.step(np.array([d[s] if s < len(d) else 0.0 for d in datas]), np.ones(S), None, act)
            assert not rc.any(), rc
            last[act == 1] = l[act == 1]
        for k in range(S):
            assert last[k] == ll[k], k
            np.testing.assert_array_equal(fl.particles(k), fresh.particles(k))
            np.testing.assert_array_equal(fl.ancestors(k), fresh.ancestors(k))


# 6 ------------------------------------------------------------------------------------------------------------------------------
def test_filter_paths_are_a_handles():
    S, n = 5, 300
    models, seeds, datas = ragged_c4(S)
    with NativeLgcpFleet(models[0], n, S, 2) as fl:
        fl.set_params(models)
        fl.reseed(seeds)
        ll, ll_t, ess_t, paths, last, rc = fl.filter(datas)
        assert not rc.any(), rc
        ll2, _, _, none, last2, rc2 = fl.filter(datas, want_path=False)
        assert none is None and not rc2.any()
        np.testing.assert_array_equal(last2, last)
        np.testing.assert_array_equal(ll2, ll)
        for k in range(S):
            with NativePf(models[k], n, seeds[k], lgcp_precision=2) as g:
                gl, gll_t, gess_t, gpath = g.run(*events(datas[k]), want_path=True)
            assert ll[k] == gl
            np.testing.assert_array_equal(ll_t[k], gll_t)
            np.testing.assert_array_equal(ess_t[k], gess_t)
            np.testing.assert_array_equal(paths[k], gpath)
            np.testing.assert_array_equal(last[k], gpath[-1])


# 7 ------------------------------------------------------------------------------------------------------------------------------
def test_one_series_that_cannot_be_weighed():
    S, n = 5, 200
    good = cases.c4_model()
    wild = Model.lgcp(Sde.ouProcess(1)).run(Parameters.apply(None, SdeParameter.ouParameter(800, 0.5, 0.4, 800, 0.5)))
    models = [wild if k == 2 else good for k in range(S)]
    seeds = [SEED + 17 * k for k in range(S)]
    datas = [cases.event_times(5, seed=SEED + k, horizon=2.0)[0] for k in range(S)]
    o = oracle.OraclePf(wild.descriptor(2), n, seeds[2])
    o.init(float(datas[2][0]))
    o.step(float(datas[2][0]), 1.0, True)
    with pytest.raises(oracle.OracleError) as ei:
        o.step(float(datas[2][1]), 1.0, True)
    assert ei.value.code == -5
    with NativeLgcpFleet(good, n, S, 2) as fl, NativeLgcpFleet(good, n, S - 1, 2) as without:
        fl.set_params(models); fl.reseed(seeds)
        ll, ll_t, ess_t, rc = fl.ll_filter(datas)
        assert list(rc) == [0, 0, _abi.CSSM_ENONFINITE, 0, 0]
        assert np.isnan(ll[2]) and not np.isnan(ll_t[2][0]) and np.isnan(ll_t[2][1:]).all() and (ess_t[2][1:] == -1).all()
        keep = [0, 1, 3, 4]
        without.reseed([seeds[k] for k in keep])
        wl, wll_t, wess_t, wrc = without.ll_filter([datas[k] for k in keep])
        assert not wrc.any()
        for j, k in enumerate(keep):
            assert ll[k] == wl[j]
            np.testing.assert_array_equal(ll_t[k], wll_t[j])
            np.testing.assert_array_equal(ess_t[k], wess_t[j])
            np.testing.assert_array_equal(fl.particles(k), without.particles(j))
            np.testing.assert_array_equal(fl.ancestors(k), without.ancestors(j))
        _, _, rc = fl.step(np.array([d[-1] + 0.1 for d in datas]), np.ones(S))
        assert list(rc) == [0, 0, _abi.CSSM_ESTATE, 0, 0]


# 9 ------------------------------------------------------------------------------------------------------------------------------
def test_refusals_on_a_live_fleet():
    S, n, model = 3, 100, cases.c4_model()
    datas = [FIXTURE[:5] + k for k in range(S)]
    trip = [events(d) for d in datas]
    with NativeLgcpFleet(model, n, S, 2) as fl:
        fl.reseed([SEED + k for k in range(S)])
        ll0, _, _, rc = fl.ll_filter(datas)
        assert not rc.any()
        t1, y1 = np.array([d[-1] + 0.2 for d in datas]), np.ones(S)
        c2 = cases.c2_model().descriptor()
        nt = C.c_size_t()
        _abi.check(fl.lib.cssm_desc_flatten(c2.ptr(), None, 0, C.byref(nt)))
        off, t, y, has = fl.pack(datas)
        lib, h = fl.lib, fl._h
        calls = {
            "filter_intervals": lambda: fl.filter_intervals(trip),
            "step_intervals": lambda: fl.step_intervals(t1, y1),
            "filter_forecasts": lambda: fl.filter_forecasts(trip),
            "step_forecast": lambda: fl.step_forecast(t1, y1),
            "forecast": lambda: fl.forecast([[50.0]] * S),
            "forecast_posterior": lambda: _abi.check(lib.cssm_fleet_forecast_posterior(h, *([None] * 3), 0, *([None] * 6), 0.975, *([None] * 12))),
            "interpolate": lambda: fl.interpolate(trip),
            "window": lambda: fl.window(4),
            "step_interpolate": lambda: fl.step_interpolate(t1, y1),
            "simulate": lambda: fl.simulate(np.zeros(S), [[1.0]] * S),
            "pmmh_run": lambda: fl.pmmh_run(c2, np.zeros((S, nt.value)), 0.05, off, t, y, has, [1] * S, 2),
        }
        for name, call in calls.items():
            with pytest.raises(_abi.CssmError) as ei:
                call()
            assert ei.value.code == _abi.CSSM_EINVAL_ARG and "LGCP fleet" in str(ei.value) and "cssm_fleet_" + name in str(ei.value), (name, str(ei.value))
            assert ("cssm_pmmh_run_batched" if name == "pmmh_run" else "cssm_pf_") in str(ei.value), name
        # an LGCP descriptor is still refused by cssm_fleet_pmmh_run as itself, before the fleet is looked at
        with pytest.raises(_abi.CssmError) as ei:
            fl.pmmh_run(model.descriptor(2), np.zeros((S, 5)), 0.05, off, t, y, has, [1] * S, 2)
        assert ei.value.code == _abi.CSSM_EINVAL_DESC
        with pytest.raises(_abi.CssmError) as ei:
            fl.set_option(2, 1)                                           # CSSM_OPT_RESAMPLER, stratified
        assert ei.value.code == _abi.CSSM_EINVAL_ARG
        finer = model.descriptor(3)                                       # the fleet's structure holds precision 2
        arr = (_abi._descp * S)(*[C.pointer(finer.desc)] * S)
        assert lib.cssm_fleet_set_params(h, arr) == _abi.CSSM_EINVAL_DESC and b"series 0" in lib.cssm_last_error()
        # ... and the fleet still filters, to the same bits
        ll1, _, _, rc = fl.ll_filter(datas)
        assert not rc.any()
        np.testing.assert_array_equal(ll1, ll0)


# 10 -----------------------------------------------------------------------------------------------------------------------------
def test_from_the_simulator_to_the_filter():
    model, P, n = cases.c4_model(), 8, 200
    sim = simulate_lgcp(model, 0.0, 10.0, 1, n_paths=P, keep_grid=False)
    data = lgcp_fleet_data(sim)
    assert all(len(a) > 0 for a in data), [len(a) for a in data]      # (about 12 events per path: an empty one has probability ~ e^-12)
    keys = FilterFleet.keys(SEED, P)
    with NativeLgcpFleet(model, n, P, 1) as fl:
        fl.reseed(keys)
        ll, _, _, rc = fl.ll_filter(data)
        assert not rc.any(), rc
    loop = [FilterLgcp(model, Resampling.systematicResampling, 1, seed=keys[p]).llFilter(lgcp_events_data(sim, p), n) for p in range(P)]
    assert ll.tolist() == loop
    with FilterLgcpFleet([model] * P, Resampling.systematicResampling, 1, n, seed=SEED) as ff:
        assert ff.llFilter([lgcp_events_data(sim, p) for p in range(P)]).tolist() == loop
