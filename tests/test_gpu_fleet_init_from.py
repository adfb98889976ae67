"""-m gpu: fleet series started from given states and continued in batches (include/cssm_pf.h: cssm_fleet_init_from,
cssm_fleet_ll_filter_more, cssm_fleet_filter_intervals_more).  Per series the results must be those of the oracle's FilterInit
(OraclePf.init_from followed by its step loop) and of a handle of its own (cssm_pf_init_from + cssm_pf_ll_filter_more), bit for bit:
every comparison below is == / assert_array_equal, no series is skipped or excused, and every status is zero where the test does not
ask for one.  No fault is provoked anywhere: what is refused is refused on the host, and the one failing series is the documented
non-finite status of a record whose time lies before the series' clock.

Checked here because no host without a device reaches them (tests/test_fleet_init_from_host.py says so): pick_out of the draw path
against the host twin tests/cpp/posterior_pick_twin.c, and a decreasing moff / off."""
import ctypes as C

import numpy as np
import pytest

import cases
from composablestatespacemodels_amd import CssmError, Data, FilterInitFleet, _abi
from composablestatespacemodels_amd.filter import FilterFleet, FilterInit, NativeLgcpFleet, NativePf, NativePfFleet, Resampling
from composablestatespacemodels_amd.pmmh import fleet_posterior_rows, pmmh_native_fleet
from oracle import oracle
from test_fleet_init_from_host import build_pick_twin, twin_picks
from test_gpu_fleet import _perturbed, ragged_c2

pytestmark = pytest.mark.gpu

SEED = cases.SEED
EMPTY = (np.zeros(0), np.zeros(0), np.zeros(0, dtype=np.uint8))


def cut(data, a, b=None):
    return tuple(np.asarray(v)[a:b] for v in data)


def start_rows(S, d, seed=SEED):
    """one state per series: what FilterInit replicates"""
    return [np.round(np.random.default_rng(seed + k).normal(0.0, 0.7, d), 3) for k in range(S)]


def oracle_from(desc, n, seed, t0, row, data):
    """FilterInit on the oracle: init_from(t0, row), then the step loop: (handle, ll, ll_t, ess_t)"""
    o = oracle.OraclePf(desc, n, seed)
    o.init_from(float(t0), row)
    ll_t, ess_t, ll = [], [], 0.0
    for t, y, h in zip(*data):
        ll, ess = o.step(float(t), float(y), bool(h))
        ll_t.append(ll); ess_t.append(ess)
    return o, ll, np.array(ll_t), np.array(ess_t, dtype=np.int32)


def assert_cloud_equal(fa, ka, other, kb=None):
    """cloud and ancestors of series ka of fleet fa against series kb of another fleet, or against an oracle / handle"""
    xb, ab = (other.particles(kb), other.ancestors(kb)) if kb is not None else (other.particles(), other.ancestors())
    np.testing.assert_array_equal(fa.particles(ka), xb)
    np.testing.assert_array_equal(fa.ancestors(ka), ab)


def assert_series_is_filter_init(fl, k, model, n, seed, t0, row, data, ll, ll_t, ess_t, native=True, desc=None, precision=0):
    o, ol, oll_t, oess_t = oracle_from(desc or model.descriptor(), n, seed, t0, row, data)
    assert ll[k] == ol, (k, n, ll[k], ol)
    np.testing.assert_array_equal(ll_t[k], oll_t)
    np.testing.assert_array_equal(ess_t[k], oess_t)
    assert_cloud_equal(fl, k, o)
    if native:
        with NativePf(model, n, seed, lgcp_precision=precision) as g:
            g.init_from(float(t0), row)
            gl, gll_t, gess_t = g.run_more(*data)
            assert ll[k] == gl
            np.testing.assert_array_equal(ll_t[k], gll_t)
            np.testing.assert_array_equal(ess_t[k], gess_t)
            assert_cloud_equal(fl, k, g)


# 1 ------------------------------------------------------------------------------------------------------------------------------
def _filter_init_case(models, seeds, datas, n):
    S, d = len(models), None
    with NativePfFleet(models[0], n, S) as fl:
        d = fl.d
        fl.set_params(models); fl.reseed(seeds)
        rows = start_rows(S, d)
        t0 = np.array([datas[k][0][0] - 0.25 * (k % 3) for k in range(S)])      # (a first increment of 0 among them)
        pick_out, rc = fl.init_from(t0, rows)
        assert not rc.any() and not pick_out.any(), rc
        for k in range(S):                                   # the row in every column, identity ancestors, nothing observed yet
            np.testing.assert_array_equal(fl.particles(k), np.repeat(rows[k][:, None], n, axis=1))
            np.testing.assert_array_equal(fl.ancestors(k), np.arange(n, dtype=np.uint32))
            assert fl.observation_index(k) == 0
        ll, ll_t, ess_t, rc = fl.ll_filter_more(datas)
        assert not rc.any(), rc
        for k in range(S):
            assert fl.observation_index(k) == len(datas[k][0])
            assert_series_is_filter_init(fl, k, models[k], n, seeds[k], t0[k], rows[k], datas[k], ll, ll_t, ess_t)
        assert fl.last_ms()[0] > 0.0


@pytest.mark.parametrize("n", [1, 64, 65, 100, _abi.FLEET_MAX_N])
def test_filter_init_per_series(n):
    assert _abi.FLEET_MAX_N == 4096
    _filter_init_case(*ragged_c2(6), n)


@pytest.mark.parametrize("d", [1, 16])
def test_filter_init_per_series_at_the_ends_of_the_dimensions(d):
    S = 3
    _filter_init_case([cases.dim_model(d)] * S, [SEED + 17 * k for k in range(S)], [cases.poisson_counts(6 + k, seed=SEED + k) for k in range(S)], 65)


# 2 ------------------------------------------------------------------------------------------------------------------------------
def _ll_filter_some(fl, datas):
    """ll_filter of the series that have records; the others keep what they hold (their status says they had none)"""
    ll, ll_t, ess_t, rc = fl.ll_filter_packed(*fl.pack(datas, allow_empty=True))
    assert [int(v) for v in rc] == [0 if len(d[0]) else _abi.CSSM_EINVAL_ARG for d in datas], rc
    return ll, ll_t, ess_t


def _split_case(make, models, seeds, datas, splits, lgcp=False):
    S = len(datas)
    tmin = np.array([np.min(d[0]) for d in datas])
    pre = [cut(datas[k], 0, splits[k]) for k in range(S)]
    post = [cut(datas[k], splits[k]) for k in range(S)]
    with make() as whole, make() as two, make() as loop:
        for fl in (whole, two, loop):
            if models is not None:
                fl.set_params(models)
            fl.reseed(seeds)
        wl, wll_t, wess_t, rc = whole.ll_filter(datas)
        assert not rc.any(), rc
        for fl in (two, loop):
            fl.init(tmin)                                     # a series split at 0 holds the cloud ll_filter would have drawn, at its clock
            _, pll_t, pess_t = _ll_filter_some(fl, pre)
        ll, ll_t, ess_t, rc = two.ll_filter_more(post)
        assert not rc.any(), rc
        for k in range(S):
            if splits[k] < len(datas[k][0]):
                assert ll[k] == wl[k], (k, ll[k], wl[k])
            else:
                assert np.isnan(ll[k])                        # continued by nothing: not written
            np.testing.assert_array_equal(np.concatenate([pll_t[k], ll_t[k]]), wll_t[k])
            np.testing.assert_array_equal(np.concatenate([pess_t[k], ess_t[k]]), wess_t[k])
            assert two.observation_index(k) == len(datas[k][0])
            assert_cloud_equal(two, k, whole, k)
        # ... and the loop of cssm_fleet_step over the same records
        for r in range(max(len(p[0]) for p in post)):
            active = np.array([r < len(post[k][0]) for k in range(S)], dtype=np.uint8)
            col = lambda j, ty: np.array([post[k][j][r] if active[k] else 0 for k in range(S)], dtype=ty)
            sl, se, rc = loop.step(col(0, np.float64), col(1, np.float64), None if lgcp else col(2, np.uint8), active)
            assert not rc.any(), (r, rc)
            for k in range(S):
                if active[k]:
                    assert (sl[k], se[k]) == (ll_t[k][r], ess_t[k][r]), (r, k)
        for k in range(S):
            assert_cloud_equal(two, k, loop, k)


def test_split_identities():
    S, n = 6, 257
    models, seeds, datas = ragged_c2(S)
    T = [len(d[0]) for d in datas]
    gap = int(np.flatnonzero(datas[1][2] == 0)[0])            # series 1's first record without a datum: the second call starts with it
    assert datas[1][2][gap] == 0 and 0 < gap < T[1]
    make = lambda: NativePfFleet(models[0], n, S)
    for splits in ([1] * S, [t - 1 for t in T], [0, gap, T[2], 3, 0, T[5]], [T[0], gap + 1, 1, 0, 2, 4]):
        _split_case(make, models, seeds, datas, splits)


@pytest.mark.parametrize("name,precision", [("c4_model", 2), ("lgcp_seasonal_model", 1)])
def test_split_identities_on_an_lgcp_fleet(name, precision):
    model, S, n = getattr(cases, name)(), 3, 100
    seeds = [SEED + 17 * k for k in range(S)]
    datas = [cases.event_times(5 + 2 * k, seed=SEED + k, horizon=2.0) for k in range(S)]
    make = lambda: NativeLgcpFleet(model, n, S, precision)
    for splits in ([1, 3, 8], [0, 2, 9], [5, 6, 0]):
        _split_case(make, None, seeds, datas, splits, lgcp=True)


# 3 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [65, 1000])
def test_filter_intervals_more_equals_the_loop_of_step_intervals(n):
    S = 5
    models, seeds, datas = ragged_c2(S)
    splits = [2, 0, 3, len(datas[3][0]), 1]
    tmin = np.array([np.min(d[0]) for d in datas])
    pre = [cut(datas[k], 0, splits[k]) for k in range(S)]
    post = [cut(datas[k], splits[k]) for k in range(S)]
    for interval in (0.975, 0.5):
        with NativePfFleet(models[0], n, S) as fa, NativePfFleet(models[0], n, S) as fb, NativePfFleet(models[0], n, S) as fc:
            for fl in (fa, fb, fc):
                fl.set_params(models); fl.reseed(seeds); fl.init(tmin)
                _ll_filter_some(fl, pre)
            ll, ll_t, ess_t, rows, rc = fa.filter_intervals_more(post, interval)
            assert not rc.any(), rc
            cl, cll_t, cess_t, rc = fc.ll_filter_more(post)
            assert not rc.any(), rc
            np.testing.assert_array_equal(ll, cl)             # (NaN where a series was continued by nothing)
            for k in range(S):
                np.testing.assert_array_equal(ll_t[k], cll_t[k]); np.testing.assert_array_equal(ess_t[k], cess_t[k])
                assert_cloud_equal(fa, k, fc, k)
                assert all(len(a) == len(post[k][0]) for a in rows[k])
            for r in range(max(len(p[0]) for p in post)):
                active = np.array([r < len(post[k][0]) for k in range(S)], dtype=np.uint8)
                col = lambda j, ty: np.array([post[k][j][r] if active[k] else 0 for k in range(S)], dtype=ty)
                sl, se, srows, rc = fb.step_intervals(col(0, np.float64), col(1, np.float64), col(2, np.uint8), active, interval)
                assert not rc.any(), (r, rc)
                for k in range(S):
                    if active[k]:
                        assert (sl[k], se[k]) == (ll_t[k][r], ess_t[k][r]), (r, k)
                        for a, b in zip(rows[k], srows):      # order statistics and means alike: the same statements, the same order
                            np.testing.assert_array_equal(a[r], b[k], err_msg=f"interval {interval} record {r} series {k}")
            assert fa.last_ms()[0] > 0.0


def test_filter_intervals_more_refuses_an_lgcp_fleet_which_then_filters_as_ever():
    model, S, n = cases.c4_model(), 3, 100
    seeds = [SEED + 17 * k for k in range(S)]
    datas = [cases.event_times(5 + 2 * k, seed=SEED + k, horizon=2.0) for k in range(S)]
    with NativeLgcpFleet(model, n, S, 2) as fl, NativeLgcpFleet(model, n, S, 2) as twin:
        fl.reseed(seeds); twin.reseed(seeds)
        fl.init(0.0)
        with pytest.raises(CssmError) as e:
            fl.filter_intervals_more(datas)
        assert e.value.code == _abi.CSSM_EINVAL_ARG and "LGCP fleet" in str(e.value) and "cssm_fleet_filter_intervals_more" in str(e.value)
        a, b = fl.ll_filter(datas), twin.ll_filter(datas)
        assert not a[3].any() and not b[3].any()
        np.testing.assert_array_equal(a[0], b[0])
        for k in range(S):
            np.testing.assert_array_equal(a[1][k], b[1][k]); np.testing.assert_array_equal(a[2][k], b[2][k])
            assert_cloud_equal(fl, k, twin, k)


# 4 ------------------------------------------------------------------------------------------------------------------------------
def test_posterior_start_with_drawn_picks(tmp_path):
    n, S = 65, 4
    Ms = [2, 3, n, 3 * n + 1]
    um = cases.c2_unparam()
    params = [_perturbed(cases.c2_params, k) for k in range(S)]
    models = [um.run(p) for p in params]
    keys = [0x0B5E55ED + 977 * k for k in range(S)]
    rng = np.random.default_rng(SEED)
    xs = [np.round(rng.normal(0.0, 1.0, (M, 3)), 4) for M in Ms]
    t0 = np.array([0.5 * k for k in range(S)])
    twin = build_pick_twin(tmp_path)
    with NativePfFleet(models[0], n, S) as fl:
        fl.set_params(models); fl.reseed([SEED + k for k in range(S)])
        pick_out, rc = fl.init_from(t0, xs, keys=keys)
        assert not rc.any(), rc
        post = [(np.tile(np.asarray(params[k].flattenParams()), (Ms[k], 1)), xs[k]) for k in range(S)]
        fc = fl.forecast_posterior(post, t0, [[t0[k] + 1.0] for k in range(S)], keys=keys)
        for k in range(S):
            assert fc[k]["rc"] == 0
            np.testing.assert_array_equal(pick_out[k], fc[k]["pick"])
            np.testing.assert_array_equal(pick_out[k], twin_picks(twin, keys[k], n, Ms[k]))
            assert pick_out[k].max() < Ms[k] and len(set(pick_out[k].tolist())) > 1
            np.testing.assert_array_equal(fl.particles(k), xs[k][pick_out[k]].T)      # the forecast did not touch the clouds
            np.testing.assert_array_equal(fl.ancestors(k), np.arange(n, dtype=np.uint32))


# 5 ------------------------------------------------------------------------------------------------------------------------------
def test_posterior_start_the_gather_is_the_only_difference():
    n, S, d = 65, 3, 3
    model, seed = cases.c2_model(), SEED + 5
    rng = np.random.default_rng(SEED + 1)
    X = np.round(rng.normal(0.0, 1.0, (3, d)), 4)
    p = rng.integers(0, 3, n).astype(np.uint32)
    assert set(p.tolist()) == {0, 1, 2}
    ident = np.arange(n, dtype=np.uint32)
    data = cases.poisson_counts(9, seed=SEED + 2, missing=0.3)
    t, y, has = data
    assert has.any() and not has.all()
    t0 = float(t[0]) - 0.5
    with NativePfFleet(model, n, S) as fl:
        fl.reseed([seed] * S)
        # series 0: rows X under the picks p; series 1: the N rows X[p] under the identity; series 2: X[0] alone
        pick_out, rc = fl.init_from(t0, [X, X[p], X[0]], picks=np.stack([p, ident, np.zeros(n, dtype=np.uint32)]))
        assert not rc.any(), rc
        np.testing.assert_array_equal(pick_out, np.stack([p, ident, np.zeros(n, dtype=np.uint32)]))
        np.testing.assert_array_equal(fl.particles(0), X[p].T)
        assert_cloud_equal(fl, 0, fl, 1)
        # one record without a datum: column i is the oracle's column i started from the row it picked
        step1 = (t[:1], y[:1], np.zeros(1, dtype=np.uint8))
        ll, ll_t, ess_t, rc = fl.ll_filter_more([step1] * S)
        assert not rc.any() and list(ll) == [0.0] * S
        assert_cloud_equal(fl, 0, fl, 1)
        got = fl.particles(0)
        for m in range(3):
            o = oracle.OraclePf(model.descriptor(), n, seed)
            o.init_from(t0, X[m])
            o.step(float(t[0]), 0.0, False)
            np.testing.assert_array_equal(got[:, p == m], o.particles()[:, p == m])
        # ... and weighted and unweighted records behind it
        ll, ll_t, ess_t, rc = fl.ll_filter_more([cut(data, 1)] * S)
        assert not rc.any(), rc
        assert ll[0] == ll[1]
        np.testing.assert_array_equal(ll_t[0], ll_t[1]); np.testing.assert_array_equal(ess_t[0], ess_t[1])
        assert_cloud_equal(fl, 0, fl, 1)
        # all rows equal: both are the M = 1 start, and so the oracle's FilterInit
        same = np.repeat(X[:1], 3, axis=0)
        _, rc = fl.init_from(t0, [same, same[p], X[0]], picks=np.stack([p, ident, np.zeros(n, dtype=np.uint32)]))
        assert not rc.any(), rc
        ll, ll_t, ess_t, rc = fl.ll_filter_more([data] * S)
        assert not rc.any(), rc
        for k in range(S):
            assert_series_is_filter_init(fl, k, model, n, seed, t0, X[0], data, ll, ll_t, ess_t, native=k == 0)


# 6 ------------------------------------------------------------------------------------------------------------------------------
def test_selective_restart():
    S, n = 5, 100
    models, seeds, datas = ragged_c2(S)
    splits = [2, 3, 1, 2, 4]
    pre = [cut(datas[k], 0, splits[k]) for k in range(S)]
    post = [cut(datas[k], splits[k]) for k in range(S)]
    restart = np.array([0, 1, 0, 1, 0], dtype=np.uint8)
    rows = start_rows(S, 3, SEED + 9)
    t0 = np.array([post[k][0][0] - 0.125 for k in range(S)])
    with NativePfFleet(models[0], n, S) as fl, NativePfFleet(models[0], n, S) as calm:
        for f in (fl, calm):
            f.set_params(models); f.reseed(seeds)
            _, _, _, rc = f.ll_filter(pre)
            assert not rc.any()
        junk = [np.full(3, np.nan) if not restart[k] else rows[k] for k in range(S)]      # (nothing of an inactive series is read)
        pick_out, rc = fl.init_from(np.where(restart != 0, t0, np.nan), junk, active=restart)
        assert not rc.any() and not pick_out.any(), rc
        for k in range(S):
            assert fl.observation_index(k) == (0 if restart[k] else splits[k])
        ll, ll_t, ess_t, rc = fl.ll_filter_more(post)
        cl, cll_t, cess_t, crc = calm.ll_filter_more(post)
        assert not rc.any() and not crc.any()
        for k in range(S):
            if restart[k]:
                assert_series_is_filter_init(fl, k, models[k], n, seeds[k], t0[k], rows[k], post[k], ll, ll_t, ess_t)
            else:
                assert ll[k] == cl[k]
                np.testing.assert_array_equal(ll_t[k], cll_t[k]); np.testing.assert_array_equal(ess_t[k], cess_t[k])
                assert_cloud_equal(fl, k, calm, k)


def test_selective_restart_restarts_the_window():
    S, n = 5, 100
    models, seeds, datas = ragged_c2(S)
    restart = np.array([0, 1, 0, 1, 0], dtype=np.uint8)
    rows = start_rows(S, 3, SEED + 9)
    col = lambda r, j, ty: np.array([datas[k][j][r] for k in range(S)], dtype=ty)
    with NativePfFleet(models[0], n, S) as fl, NativePfFleet(models[0], n, S) as fresh:
        for f in (fl, fresh):
            f.set_params(models); f.reseed(seeds); f.window(4)
        fl.init(col(0, 0, np.float64))
        for r in range(3):
            _, _, nrows, _, rc = fl.step_interpolate(col(r, 0, np.float64), col(r, 1, np.float64), col(r, 2, np.uint8), lag=3, max_lag=3)
            assert not rc.any()
        assert [fl.window_depth(k) for k in range(S)] == [3] * S
        t0 = col(3, 0, np.float64) - 0.125
        for f in (fl, fresh):
            _, rc = f.init_from(t0, rows, active=restart)
            assert not rc.any()
        assert [fl.window_depth(k) for k in range(S)] == [0 if restart[k] else 3 for k in range(S)]
        args = (col(3, 0, np.float64), col(3, 1, np.float64), col(3, 2, np.uint8))
        la, ea, na, ra, rc = fl.step_interpolate(*args, lag=3, max_lag=3)
        assert not rc.any()
        lb, eb, nb, rb, rc = fresh.step_interpolate(*args, active=restart, lag=3, max_lag=3)
        assert list(rc) == [0] * S
        for k in range(S):
            if not restart[k]:
                assert na[k] == 4 and fl.window_depth(k) == 3
                continue
            assert na[k] == nb[k] == 2 and fl.window_depth(k) == 1      # the base slice and the record: as behind cssm_fleet_init
            assert (la[k], ea[k]) == (lb[k], eb[k])
            for a, b in zip(ra, rb):
                np.testing.assert_array_equal(a[k], b[k])


# 7 ------------------------------------------------------------------------------------------------------------------------------
def _raw_init_from(fl, t0, moff, x, rc):
    p = lambda a, ty: a.ctypes.data_as(C.POINTER(ty))
    return fl.lib.cssm_fleet_init_from(fl._h, None, p(t0, C.c_double), p(moff, C.c_uint64), p(x, C.c_double), None, None, None, p(rc, C.c_int))


def test_per_series_refusals_on_a_live_fleet():
    S, n = 5, 65
    models, seeds, datas = ragged_c2(S)
    splits = [2, 3, 1, 2, 4]
    pre = [cut(datas[k], 0, splits[k]) for k in range(S)]
    post = [cut(datas[k], splits[k]) for k in range(S)]
    X = np.round(np.random.default_rng(SEED).normal(0.0, 1.0, (3, 3)), 4)
    t0 = np.array([post[k][0][0] - 0.125 for k in range(S)])
    pk = np.zeros((S, n), dtype=np.uint32); pk[3] = np.arange(n) % 3
    with NativePfFleet(models[0], n, S) as fl, NativePfFleet(models[0], n, S) as calm:
        for f in (fl, calm):
            f.set_params(models); f.reseed(seeds)
            assert not f.ll_filter(pre)[3].any()
        # picks given, no keys: no rows | a NaN entry | a pick at M | served from three rows | served from one
        nan_row = X[:2].copy(); nan_row[1, 2] = np.nan
        bad = pk.copy(); bad[2, 7] = 3
        pick_out, rc = fl.init_from(t0, [None, nan_row, X, X, X[1]], picks=bad)
        assert list(rc) == [_abi.CSSM_EINVAL_ARG] * 3 + [0, 0]
        assert b"series 0:" in fl.lib.cssm_last_error()
        assert not pick_out[:3].any() and np.array_equal(pick_out[3], pk[3]) and not pick_out[4].any()
        np.testing.assert_array_equal(fl.particles(3), X[pk[3]].T)
        np.testing.assert_array_equal(fl.particles(4), np.repeat(X[1][:, None], n, axis=1))
        for k in range(3):
            assert fl.observation_index(k) == splits[k]
            assert_cloud_equal(fl, k, calm, k)
        # neither picks nor keys: two rows cannot be chosen among | one row needs neither
        act = np.array([1, 1, 0, 0, 0], dtype=np.uint8)
        pick_out, rc = fl.init_from(t0, [X[:2], X[2], None, None, None], active=act)
        assert list(rc) == [_abi.CSSM_EINVAL_ARG, 0, 0, 0, 0] and b"series 0:" in fl.lib.cssm_last_error() and b"keys" in fl.lib.cssm_last_error()
        np.testing.assert_array_equal(fl.particles(1), np.repeat(X[2][:, None], n, axis=1))
        # a non-finite t0
        _, rc = fl.init_from(np.array([np.inf, 0, 0, 0, 0]), [X[0], None, None, None, None], active=np.array([1, 0, 0, 0, 0], dtype=np.uint8))
        assert list(rc) == [_abi.CSSM_EINVAL_ARG, 0, 0, 0, 0]
        # the refused series go on as if nothing had been asked; their neighbours are the FilterInit they were made
        ll, ll_t, ess_t, rc = fl.ll_filter_more(post)
        cl, cll_t, cess_t, crc = calm.ll_filter_more(post)
        assert not rc.any() and not crc.any()
        for k in (0, 2):
            assert ll[k] == cl[k]
            np.testing.assert_array_equal(ll_t[k], cll_t[k]); np.testing.assert_array_equal(ess_t[k], cess_t[k])
            assert_cloud_equal(fl, k, calm, k)
        assert_series_is_filter_init(fl, 1, models[1], n, seeds[1], t0[1], X[2], post[1], ll, ll_t, ess_t)
        assert_series_is_filter_init(fl, 4, models[4], n, seeds[4], t0[4], X[1], post[4], ll, ll_t, ess_t)
        # a decreasing moff / off is the call's own refusal (S is the fleet's: tests/test_fleet_init_from_host.py cannot reach it)
        rcs = np.zeros(S, dtype=np.int32)
        assert _raw_init_from(fl, t0, np.array([0, 1, 2, 1, 2, 3], dtype=np.uint64), np.zeros((3, 3)), rcs) == _abi.CSSM_EINVAL_ARG
        assert b"moff must be non-decreasing" in fl.lib.cssm_last_error()
        off = np.array([0, 1, 2, 1, 2, 3], dtype=np.uint64)
        p = lambda a, ty=C.c_double: a.ctypes.data_as(C.POINTER(ty))
        z, out = np.zeros(3), np.zeros(S)
        assert fl.lib.cssm_fleet_ll_filter_more(fl._h, p(off, C.c_uint64), p(z), p(z), None, p(out), None, None, p(rcs, C.c_int)) == _abi.CSSM_EINVAL_ARG
        assert b"off must be non-decreasing" in fl.lib.cssm_last_error()
        assert fl.lib.cssm_fleet_filter_intervals_more(fl._h, p(off, C.c_uint64), p(z), p(z), None, 0.975, p(out), None, None, None, None, None, None,
                                                       None, None, p(rcs, C.c_int)) == _abi.CSSM_EINVAL_ARG
        assert b"off must be non-decreasing" in fl.lib.cssm_last_error()
        for k in (0, 2):                                     # ... and changed nothing
            assert_cloud_equal(fl, k, calm, k)


def test_continuing_without_a_cloud_is_estate():
    S, n = 3, 65
    model = cases.c2_model()
    datas = [cases.poisson_counts(4 + k, seed=SEED + k) for k in range(S)]
    seeds = [SEED + 17 * k for k in range(S)]
    row = np.array([0.1, -0.2, 0.3])
    with NativePfFleet(model, n, S) as fl:
        fl.reseed(seeds)
        for call in (fl.ll_filter_more, fl.filter_intervals_more):
            with pytest.raises(CssmError) as e:                # no series of the fleet has a cloud: the call's own status
                call(datas)
            assert e.value.code == _abi.CSSM_ESTATE
        _, rc = fl.init_from(0.0, [row, None, None], active=np.array([1, 0, 0], dtype=np.uint8))
        assert not rc.any()
        ll, ll_t, ess_t, rows, rc = fl.filter_intervals_more([datas[0], datas[1], EMPTY])
        assert list(rc) == [0, _abi.CSSM_ESTATE, 0]
        assert np.isnan(ll[1]) and np.isnan(ll_t[1]).all() and (ess_t[1] == -1).all() and all(np.isnan(a).all() for a in rows[1])
        assert np.isnan(ll[2]) and fl.observation_index(1) == 0 and fl.observation_index(2) == 0
        assert not any(np.isnan(a).any() for a in rows[0])
        assert_series_is_filter_init(fl, 0, model, n, seeds[0], 0.0, row, datas[0], ll, ll_t, ess_t)
        ll2, ll_t2, ess_t2, rc = fl.ll_filter_more([EMPTY, datas[1], EMPTY])
        assert list(rc) == [0, _abi.CSSM_ESTATE, 0] and np.isnan(ll2).all()
        with pytest.raises(CssmError) as e:                    # nothing of series 1 was made: it still has no cloud to step
            fl.particles(1)
        assert e.value.code == _abi.CSSM_ESTATE


def test_a_series_that_fails_mid_batch_is_made_whole_by_init_from():
    S, n = 3, 65
    model = cases.c2_model()
    seeds = [SEED + 17 * k for k in range(S)]
    datas = [cases.poisson_counts(6, seed=SEED + k) for k in range(S)]
    rows = start_rows(S, 3)
    tb = datas[1][0].copy(); tb[2] = -5.0                      # record 2 of series 1 lies before the series' clock
    broken = [datas[0], (tb, datas[1][1], datas[1][2]), datas[2]]
    with pytest.raises(oracle.OracleError):                    # (the premise: the oracle cannot weigh that record either)
        oracle_from(model.descriptor(), n, seeds[1], 0.0, rows[1], broken[1])
    with NativePfFleet(model, n, S) as fl:
        fl.reseed(seeds)
        _, rc = fl.init_from(0.0, rows)
        assert not rc.any()
        ll, ll_t, ess_t, irows, rc = fl.filter_intervals_more(broken)
        assert list(rc) == [0, _abi.CSSM_ENONFINITE, 0]
        assert np.isnan(ll[1]) and np.isnan(ll_t[1][2:]).all() and (ess_t[1][2:] == -1).all()
        assert not np.isnan(ll_t[1][:2]).any() and (ess_t[1][:2] > 0).all()
        for a in irows[1]:                                   # the rows of the records before the failing one stand, the others read NaN
            assert not np.isnan(a[:2]).any() and np.isnan(a[2:]).all()
        for k in (0, 2):
            assert_series_is_filter_init(fl, k, model, n, seeds[k], 0.0, rows[k], datas[k], ll, ll_t, ess_t, native=False)
        _, _, _, rc = fl.ll_filter_more([EMPTY, datas[1], EMPTY])
        assert list(rc) == [0, _abi.CSSM_ESTATE, 0]           # its cloud is undefined until it is initialised again
        _, rc = fl.init_from(0.0, rows, active=np.array([0, 1, 0], dtype=np.uint8))
        assert not rc.any()
        ll, ll_t, ess_t, rc = fl.ll_filter_more([EMPTY, datas[1], EMPTY])
        assert not rc.any()
        assert_series_is_filter_init(fl, 1, model, n, seeds[1], 0.0, rows[1], datas[1], ll, ll_t, ess_t)


# 8 ------------------------------------------------------------------------------------------------------------------------------
def _obs(data):
    return [Data(float(t), float(y) if h else None) for t, y, h in zip(*data)]


def test_filter_init_fleet_is_filter_init_per_series():
    S, n = 4, 100
    models, _, datas = ragged_c2(S)
    states = start_rows(S, 3, SEED + 3)
    obs = [_obs(d) for d in datas]
    with FilterInitFleet(models, Resampling.systematicResampling, states, n, seed=SEED) as ff:
        ll = ff.llFilter(obs)
        keys = FilterFleet.keys(SEED, S)
        for k in range(S):
            fi = FilterInit(models[k], Resampling.systematicResampling, states[k], n_particles=n, seed=keys[k])
            assert ll[k] == fi.llFilter(obs[k], n), k
            np.testing.assert_array_equal(ff._fleet.particles(k), fi._pf.particles())
            o, ol, _, _ = oracle_from(models[k].descriptor(), n, keys[k], min(d.t for d in obs[k]), states[k], datas[k])
            assert ll[k] == ol
            fi._pf.close()
        first = [o[0].t for o in obs]
        st = ff.initialiseState(first)
        assert [s.t for s in st] == first and all(s.ll == 0.0 and s.ess == n for s in st)
        for k in range(S):
            np.testing.assert_array_equal(st[k].particles, np.repeat(states[k][:, None], n, axis=1))
        outs = ff.filterIntervalsMore([o[:2] for o in obs], 0.975)
        assert [len(o) for o in outs] == [2] * S and outs[1][1].time == obs[1][1].t


def test_a_fleet_continues_from_its_own_posteriors():
    S, n, iters = 3, 100, 2
    um = cases.c2_unparam()
    inits = [_perturbed(cases.c2_params, k) for k in range(S)]
    datas = [cases.poisson_counts(6 + k, seed=SEED + k) for k in range(S)]
    obs = [_obs(d) for d in datas]
    _, theta, _, last = pmmh_native_fleet(um, inits, obs, n, 0.05, iters, [SEED + 100 + k for k in range(S)])
    post = fleet_posterior_rows(theta, last)
    t_end = [d[0][-1] for d in datas]
    nxt = [[Data(float(t_end[k]) + 1.0 + j, float(3 + j)) for j in range(2 + k)] for k in range(S)]
    with FilterFleet([um.run(p) for p in inits], Resampling.systematicResampling, n, seed=SEED) as ff:
        st = ff.initialiseStateFrom(t_end, [last_k for _, last_k in post])
        assert [s.t for s in st] == [float(v) for v in t_end]
        for k in range(S):
            x = st[k].particles
            assert x.shape == (3, n) and all(any(np.array_equal(x[:, i], r) for r in post[k][1]) for i in range(n))
        ll = ff.llFilterMore(nxt)
        assert np.isfinite(ll).all()
        for k in range(S):
            assert ff._fleet.observation_index(k) == len(nxt[k])
