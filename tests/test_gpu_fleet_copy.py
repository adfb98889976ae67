"""-m gpu: cssm_fleet_copy_series (include/cssm_pf.h, EXTENSION) -- whole series copied between the series of one fleet or from a second
fleet, on the device (k_fleet_copy).  Two properties, both bit for bit (== / assert_array_equal everywhere, no series skipped):

* identity: after ``copy_series(map)`` every served destination holds what its source held before the call (particles, ancestors,
  observation index, summary), every kept or self-mapped series what it held itself, and a second fleet that served as the source is
  unchanged;
* continuity: one ``step`` and then ``ll_filter_more`` of five records on the destination fleet give the ll, ess, clouds and ancestors of
  a TWIN fleet whose series k was created with the source's parameters and key, driven through the source's calls and then handed the
  destination's key with ``reseed`` (no reseed under ``keys=True``) -- and of a single ``NativePf`` handle driven the same way.  The ll a
  copied series carries is checked here: the step accumulates onto it.

The series are left by a ragged ``ll_filter`` at different clocks and at observation indices of both parities (LENS), so sources and
destinations sit in either half of the state buffer; N x d covers d n odd (8-byte path) and even (16-byte path), one partial tile and
many whole ones.  No fault is provoked: what is refused is refused on the host, and the one failed series is the documented non-finite
status of a record whose time lies before the series' clock.
"""
import ctypes as C

import numpy as np
import pytest

import cases
from composablestatespacemodels_amd import CssmError, UnparamModel, _abi
from composablestatespacemodels_amd.filter import NativeLgcpFleet, NativePf, NativePfFleet

pytestmark = pytest.mark.gpu

SEED = cases.SEED
S6 = 6
LENS = [3, 4, 6, 5, 2, 7]                       # records per series: observation indices of both parities
KEEP = _abi.CSSM_FLEET_COPY_KEEP
MAPS = {
    "swap": [1, 0, KEEP, KEEP, KEEP, KEEP],
    "rotation": [1, 2, 3, 4, 5, 0],             # every series is source and destination
    "all_from_0": [0, 0, 0, 0, 0, 0],
    "mix_keep": [KEEP, 0, 2, None, 1, 4],       # (2: self-mapped)
    "opposite_parity": [1, 0, 3, 2, 5, 4],      # LENS: every pair is (odd, even)
}


def base_model(d):
    return cases.c2_model() if d == 3 else cases.dim_model(d)


def series_setup(d, S=S6, lens=LENS):
    """distinct parameters, keys and ragged data per series"""
    base = base_model(d)
    um = UnparamModel([leaf[0] for leaf in base.leaves])
    th = np.asarray(base.parameters().flattenParams())
    models = [um.run(base.parameters().withFlat(th + 0.03 * (k % 7) * np.cos(np.arange(th.size) + k))) for k in range(S)]
    seeds = [SEED + 17 * k for k in range(S)]
    datas = []
    for k in range(S):
        t, y, has = cases.poisson_counts(lens[k % len(lens)], seed=SEED + k, dt=(1, .5, .25)[k % 3], missing=(0, .15, .4)[k % 3])
        datas.append((t + 3.0 * (k % 4), y, has))
    return models, seeds, datas


def drive(fl, setup, assign):
    """series k of fl created with triple assign[k]'s parameters and key and driven through its calls: the ll of every series"""
    models, seeds, datas = setup
    fl.set_params([models[j] for j in assign])
    fl.reseed([seeds[j] for j in assign])
    ll, _, _, rc = fl.ll_filter([datas[j] for j in assign])
    assert not rc.any(), rc
    return ll


def snapshot(fl, live=None):
    live = range(fl.S) if live is None else live
    return {"x": {k: fl.particles(k) for k in live}, "a": {k: fl.ancestors(k) for k in live},
            "idx": [fl.observation_index(k) for k in range(fl.S)], "summary": fl.summary(0.975), "live": set(live)}


def assert_holds(fl, k, snap, j):
    """series k of fl holds what series j held when snap was taken"""
    np.testing.assert_array_equal(fl.particles(k), snap["x"][j])
    np.testing.assert_array_equal(fl.ancestors(k), snap["a"][j])
    assert fl.observation_index(k) == snap["idx"][j]
    now = fl.summary(0.975)
    for got, was in zip(now, snap["summary"]):
        np.testing.assert_array_equal(got[k], was[j])


def effective(mp):
    return [k if (v is None or v < 0) else v for k, v in enumerate(mp)]


def continuation(setup, assign):
    """one step and five more records per series, behind the clock of the triple the series runs"""
    _, _, datas = setup
    t1 = np.array([datas[j][0][-1] + 0.5 for j in assign])
    y1 = np.array([float(2 + k % 3) for k in range(len(assign))])
    more = []
    for k in range(len(assign)):
        t, y, has = cases.poisson_counts(5, seed=SEED + 100 + k, dt=0.5, missing=0.3)
        more.append((t1[k] + 0.5 + t, y, has))
    return t1, y1, more


def assert_continue_alike(fl, tw, setup, assign):
    t1, y1, more = continuation(setup, assign)
    a, b = fl.step(t1, y1), tw.step(t1, y1)
    for u, v in zip(a, b):
        np.testing.assert_array_equal(u, v)
    assert not a[2].any(), a[2]
    (all_, allt, aess, arc), (bll, bllt, bess, brc) = fl.ll_filter_more(more), tw.ll_filter_more(more)
    np.testing.assert_array_equal(all_, bll)
    np.testing.assert_array_equal(arc, brc)
    assert not arc.any(), arc
    for k in range(fl.S):
        np.testing.assert_array_equal(allt[k], bllt[k])
        np.testing.assert_array_equal(aess[k], bess[k])
        np.testing.assert_array_equal(fl.particles(k), tw.particles(k))
        np.testing.assert_array_equal(fl.ancestors(k), tw.ancestors(k))
        assert fl.observation_index(k) == tw.observation_index(k)
    return a, (all_, allt, aess)


def same_fleet_case(d, n, mp, keys=False, make=None, setup=None):
    make = make or (lambda: NativePfFleet(base_model(d), n, S6))
    setup = setup or series_setup(d)
    ident = list(range(S6))
    eff = effective(mp)
    with make() as fl, make() as tw:
        drive(fl, setup, ident)
        snap = snapshot(fl)
        rc = fl.copy_series(mp, keys=keys)
        assert not rc.any(), rc
        assert fl.last_ms()[0] >= 0.0
        for k in range(S6):
            assert_holds(fl, k, snap, eff[k])
        drive(tw, setup, eff)
        if not keys:
            tw.reseed(setup[1])                        # the destination keeps its own key
        else:
            assert fl.seeds == [setup[1][j] for j in eff]
        assert_continue_alike(fl, tw, setup, eff)


# 1 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 65, 1000, 4096])
@pytest.mark.parametrize("d", [1, 3, 16])
def test_every_map_within_one_fleet(d, n):
    """d n odd (d odd and n odd: the 8-byte path) and even (the 16-byte path); n = 1: one partial tile; d n = 65536: 32 whole tiles"""
    for name, mp in MAPS.items():
        same_fleet_case(d, n, mp, keys=(name == "rotation" and n == 65))


def test_keys_travel_only_when_asked():
    same_fleet_case(3, 100, MAPS["rotation"], keys=True)
    same_fleet_case(3, 100, MAPS["mix_keep"], keys=True)


# 2 ------------------------------------------------------------------------------------------------------------------------------
def test_rotation_over_many_series_and_blocks():
    """S = 64 at N = 4096, d = 3: six tiles per cloud, and every live half is read while its series is written"""
    S, n = 64, 4096
    setup = series_setup(3, S)
    rot = [(k + 1) % S for k in range(S)]
    with NativePfFleet(cases.c2_model(), n, S) as fl, NativePfFleet(cases.c2_model(), n, S) as tw:
        drive(fl, setup, list(range(S)))
        snap = snapshot(fl)
        assert not fl.copy_series(rot).any()
        for k in range(S):
            assert_holds(fl, k, snap, rot[k])
        drive(tw, setup, rot)
        tw.reseed(setup[1])
        t1, y1, _ = continuation(setup, rot)
        for u, v in zip(fl.step(t1, y1), tw.step(t1, y1)):
            np.testing.assert_array_equal(u, v)
        for k in range(S):
            np.testing.assert_array_equal(fl.particles(k), tw.particles(k))
            np.testing.assert_array_equal(fl.ancestors(k), tw.ancestors(k))


# 3 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,n", [(3, 65), (1, 1000), (16, 4096)])
def test_from_a_second_fleet(d, n):
    setup = series_setup(d)
    ident, other = list(range(S6)), [(k + 3) % S6 for k in range(S6)]
    mp = [2, KEEP, 2, 0, 4, 5]                          # (4: the same index of the OTHER fleet is a copy like any other)
    with NativePfFleet(base_model(d), n, S6) as fl, NativePfFleet(base_model(d), n, S6) as src, NativePfFleet(base_model(d), n, S6) as tw:
        drive(fl, setup, ident)
        drive(src, setup, other)
        mine, theirs = snapshot(fl), snapshot(src)
        assert not fl.copy_series(mp, src=src).any()
        for k in range(S6):
            if mp[k] == KEEP:
                assert_holds(fl, k, mine, k)
            else:
                assert_holds(fl, k, theirs, mp[k])
            assert_holds(src, k, theirs, k)             # the source fleet is as it was
        assign = [k if mp[k] == KEEP else other[mp[k]] for k in range(S6)]
        drive(tw, setup, assign)
        tw.reseed(setup[1])
        assert_continue_alike(fl, tw, setup, assign)
        # ... and the source fleet continues as if nothing had read it
        with NativePfFleet(base_model(d), n, S6) as tw2:
            drive(tw2, setup, other)
            assert_continue_alike(src, tw2, setup, other)


# 4 ------------------------------------------------------------------------------------------------------------------------------
def test_a_copied_series_is_a_single_handle_reseeded_mid_series():
    n = 65
    setup = series_setup(3)
    models, seeds, datas = setup
    rot = MAPS["rotation"]
    t1, y1, more = continuation(setup, rot)
    with NativePfFleet(cases.c2_model(), n, S6) as fl:
        drive(fl, setup, list(range(S6)))
        assert not fl.copy_series(rot).any()
        ll1, ess1, rc = fl.step(t1, y1)
        assert not rc.any()
        ll, ll_t, ess_t, rc = fl.ll_filter_more(more)
        assert not rc.any()
        for k in range(S6):
            j = rot[k]
            with NativePf(models[j], n, seeds[j]) as g:
                g.run(*datas[j])
                g.reseed(seeds[k])
                gl1, gess1 = g.step(float(t1[k]), float(y1[k]))
                assert (ll1[k], ess1[k]) == (gl1, gess1)
                gl, gll_t, gess_t = g.run_more(*more[k])
                assert ll[k] == gl
                np.testing.assert_array_equal(ll_t[k], gll_t)
                np.testing.assert_array_equal(ess_t[k], gess_t)
                np.testing.assert_array_equal(fl.particles(k), g.particles())
                np.testing.assert_array_equal(fl.ancestors(k), g.ancestors())


def test_forecast_from_a_copied_series_is_the_twins():
    n = 100
    setup = series_setup(3)
    mp = MAPS["mix_keep"]
    eff = effective(mp)
    for keys in (False, True):
        with NativePfFleet(cases.c2_model(), n, S6) as fl, NativePfFleet(cases.c2_model(), n, S6) as tw:
            drive(fl, setup, list(range(S6)))
            assert not fl.copy_series(mp, keys=keys).any()
            drive(tw, setup, eff)
            if not keys:
                tw.reseed(setup[1])
            times = [setup[2][j][0][-1] + np.array([0.5, 1.0, 2.5]) for j in eff]
            for a, b in zip(fl.forecast(times), tw.forecast(times)):      # (the default keys: seed and observation index of the series)
                assert a["rc"] == b["rc"] == 0 and a["key"] == b["key"]
                for name in a:
                    if isinstance(a[name], np.ndarray):
                        np.testing.assert_array_equal(a[name], b[name])


def test_the_window_of_a_moved_series_restarts():
    n = 65
    setup = series_setup(3)
    mp = MAPS["mix_keep"]
    with NativePfFleet(cases.c2_model(), n, S6) as fl:
        drive(fl, setup, list(range(S6)))
        fl.window(4)
        t = np.array([d[0][-1] for d in setup[2]])
        for s in range(3):
            t = t + 0.5
            rc = fl.step_interpolate(t, np.full(S6, 2.0), max_lag=1)[-1]
            assert not rc.any()
        assert [fl.window_depth(k) for k in range(S6)] == [3] * S6      # three records behind the base slice (slices - 1 at the most)
        assert not fl.copy_series(mp).any()
        moved = [v is not None and v >= 0 and v != k for k, v in enumerate(mp)]
        assert moved == [False, True, False, False, True, True]
        assert [fl.window_depth(k) for k in range(S6)] == [0 if m else 3 for m in moved]


# 5 ------------------------------------------------------------------------------------------------------------------------------
def lgcp_setup(S):
    from composablestatespacemodels_amd import Model, Sde
    um = Model.lgcp(Sde.ouProcess(1))
    th = np.asarray(cases.c4_model().parameters().flattenParams())
    models = [um.run(cases.c4_model().parameters().withFlat(th + 0.03 * (k % 7) * np.cos(np.arange(th.size) + k))) for k in range(S)]
    seeds = [SEED + 17 * k for k in range(S)]
    datas = [cases.event_times(3 + k, seed=SEED + k, horizon=2.0)[0] for k in range(S)]
    return models, seeds, datas


@pytest.mark.parametrize("keys", [False, True])
def test_lgcp_fleet_copy_then_step(keys):
    """C4, S = 4, N = 65: the predicted level of the next event travels with the scalars"""
    S, n = 4, 65
    setup = lgcp_setup(S)
    models, seeds, datas = setup
    mp = [1, 2, 3, 0]
    with NativeLgcpFleet(models[0], n, S, 2) as fl, NativeLgcpFleet(models[0], n, S, 2) as tw:
        drive(fl, setup, list(range(S)))
        snap = snapshot(fl)
        assert not fl.copy_series(mp, keys=keys).any()
        for k in range(S):
            assert_holds(fl, k, snap, mp[k])
        drive(tw, setup, mp)
        if not keys:
            tw.reseed(seeds)
        t1 = np.array([datas[j][-1] + 0.125 for j in mp])
        for u, v in zip(fl.step(t1, np.ones(S)), tw.step(t1, np.ones(S))):
            np.testing.assert_array_equal(u, v)
        more = [t1[k] + np.cumsum([0.1, 0.2, 0.05, 0.3, 0.15]) for k in range(S)]
        (all_, allt, aess, arc), (bll, bllt, bess, brc) = fl.ll_filter_more(more), tw.ll_filter_more(more)
        assert not arc.any() and not brc.any()
        np.testing.assert_array_equal(all_, bll)
        for k in range(S):
            np.testing.assert_array_equal(allt[k], bllt[k])
            np.testing.assert_array_equal(aess[k], bess[k])
            np.testing.assert_array_equal(fl.particles(k), tw.particles(k))
            np.testing.assert_array_equal(fl.ancestors(k), tw.ancestors(k))


# 6 ------------------------------------------------------------------------------------------------------------------------------
def raw_copy(dst, src, mp, flags=0):
    mp = np.ascontiguousarray(mp, dtype=np.int64)
    rc = np.full(dst.S, 77, dtype=np.int32)
    got = dst.lib.cssm_fleet_copy_series(dst._h, src._h, mp.ctypes.data_as(C.POINTER(C.c_uint64)), flags, rc.ctypes.data_as(C.POINTER(C.c_int)))
    return got, rc


def assert_untouched(fl, snap):
    for k in range(fl.S):
        assert_holds(fl, k, snap, k)


def test_whole_call_refusals_change_nothing():
    n = 65
    setup = series_setup(3)
    ident = list(range(S6))
    with NativePfFleet(cases.c2_model(), n, S6) as fl:
        drive(fl, setup, ident)
        snap = snapshot(fl)
        for bad in ([S6, 0, 1, 2, 3, 4], [0, 1, 2, 3, 4, -2], [0, 1, 2, 3, 4, 1 << 40]):
            got, rc = raw_copy(fl, fl, bad)
            assert got == _abi.CSSM_EINVAL_ARG and "map[" in _abi.last_error() and (rc == 77).all()
            assert_untouched(fl, snap)
        with pytest.raises(CssmError) as e:
            fl.copy_series([S6, 0, 1, 2, 3, 4])
        assert e.value.code == _abi.CSSM_EINVAL_ARG
        got, rc = raw_copy(fl, fl, MAPS["rotation"], flags=2)
        assert got == _abi.CSSM_EINVAL_ARG and "flag" in _abi.last_error() and (rc == 77).all()
        got, rc = raw_copy(fl, fl, MAPS["rotation"], flags=_abi.CSSM_FLEET_COPY_KEYS | 4)
        assert got == _abi.CSSM_EINVAL_ARG
        assert_untouched(fl, snap)
        with NativePfFleet(cases.c2_model(), n - 1, S6) as other:                 # another N
            drive(other, setup, ident)
            got, rc = raw_copy(fl, other, MAPS["rotation"])
            assert got == _abi.CSSM_EINVAL_ARG and "particles" in _abi.last_error() and (rc == 77).all()
            assert_untouched(fl, snap)
        with NativePfFleet(cases.negbin_model(), n, 2) as other:                  # another structure (d = 3 as well)
            got, rc = raw_copy(fl, other, [0, 1, 0, 1, 0, 1])
            assert got == _abi.CSSM_EINVAL_DESC and "obs_kind" in _abi.last_error() and (rc == 77).all()
            assert_untouched(fl, snap)
        # ll, ess and the clocks stood too: the fleet continues like a twin that was never asked (the step accumulates onto ll, dt comes
        # from the clock) -- through one more copy, which the call still serves
        assert not fl.copy_series(MAPS["swap"]).any()
        assert_holds(fl, 0, snap, 1)
        assert_holds(fl, 1, snap, 0)
        eff = effective(MAPS["swap"])
        with NativePfFleet(cases.c2_model(), n, S6) as tw:
            drive(tw, setup, eff)
            tw.reseed(setup[1])
            assert_continue_alike(fl, tw, setup, eff)


def test_lgcp_into_plain_is_refused():
    n = 65
    lg = lgcp_setup(2)
    with NativePfFleet(cases.dim_model(1), n, 2) as fl, NativeLgcpFleet(lg[0][0], n, 2, 2) as ev:
        t, y, has = cases.poisson_counts(4)
        assert not fl.ll_filter([(t, y, has)] * 2)[3].any()
        drive(ev, lg, [0, 1])
        snap, snap_ev = snapshot(fl), snapshot(ev)
        got, rc = raw_copy(fl, ev, [0, 1])
        assert got == _abi.CSSM_EINVAL_ARG and "LGCP" in _abi.last_error() and (rc == 77).all()
        got, rc = raw_copy(ev, fl, [0, 1])
        assert got == _abi.CSSM_EINVAL_ARG and (rc == 77).all()
        assert_untouched(fl, snap)
        assert_untouched(ev, snap_ev)
        # ... ll, ess, clock and (LGCP) the predicted level included: either fleet steps like a twin that was never asked
        with NativePfFleet(cases.dim_model(1), n, 2) as tw, NativeLgcpFleet(lg[0][0], n, 2, 2) as tw_ev:
            assert not tw.ll_filter([(t, y, has)] * 2)[3].any()
            drive(tw_ev, lg, [0, 1])
            t1 = np.full(2, t[-1] + 0.5)
            for u, v in zip(fl.step(t1, np.full(2, 2.0)), tw.step(t1, np.full(2, 2.0))):
                np.testing.assert_array_equal(u, v)
            e1 = np.array([lg[2][k][-1] + 0.125 for k in range(2)])
            for u, v in zip(ev.step(e1, np.ones(2)), tw_ev.step(e1, np.ones(2))):
                np.testing.assert_array_equal(u, v)


def test_a_source_without_a_cloud_is_that_series_own_status():
    """series 4 never initialised, series 2 failed (a record before its clock): both as sources, and series 4 as a destination"""
    n = 65
    setup = series_setup(3)
    models, seeds, datas = setup
    empty = (np.zeros(0), np.zeros(0), np.zeros(0, dtype=np.uint8))
    with NativePfFleet(cases.c2_model(), n, S6) as fl, NativePfFleet(cases.c2_model(), n, S6) as tw:
        fl.set_params(models); fl.reseed(seeds)
        some = [empty if k == 4 else datas[k] for k in range(S6)]
        rc = fl.ll_filter_packed(*fl.pack(some, allow_empty=True))[3]
        assert [int(v) for v in rc] == [0, 0, 0, 0, _abi.CSSM_EINVAL_ARG, 0]
        active = np.zeros(S6, dtype=np.uint8); active[2] = 1
        rc = fl.step(np.full(S6, -50.0), np.full(S6, 1.0), active=active)[2]      # series 2: its record lies before its clock
        assert [int(v) for v in rc] == [0, 0, _abi.CSSM_ENONFINITE, 0, 0, 0]
        live = [0, 1, 3, 5]
        snap = snapshot(fl, live)
        mp = [4, 2, KEEP, 5, 0, 2]                      # 0 <- 4 (never initialised), 1 <- 2 and 5 <- 2 (failed), 3 <- 5, 4 <- 0 (served)
        rc = fl.copy_series(mp)
        assert [int(v) for v in rc] == [_abi.CSSM_ESTATE, _abi.CSSM_ESTATE, 0, 0, 0, _abi.CSSM_ESTATE]
        assert "series 0" in _abi.last_error() and "series 4" in _abi.last_error()
        for k in (0, 1, 5):                             # refused: exactly as they were
            assert_holds(fl, k, snap, k)
        assert_holds(fl, 3, snap, 5)
        assert_holds(fl, 4, snap, 0)
        with pytest.raises(CssmError):                  # the failed series is still without a cloud
            fl.particles(2)
        # the served and the untouched series continue like their twins
        assign = [0, 1, 2, 5, 0, 5]
        drive(tw, setup, assign)
        tw.reseed(seeds)
        t1, y1, _ = continuation(setup, assign)
        run = np.array([1, 1, 0, 1, 1, 1], dtype=np.uint8)
        for u, v in zip(fl.step(t1, y1, active=run), tw.step(t1, y1, active=run)):
            np.testing.assert_array_equal(u, v)
        for k in live + [4]:
            np.testing.assert_array_equal(fl.particles(k), tw.particles(k))
            np.testing.assert_array_equal(fl.ancestors(k), tw.ancestors(k))
