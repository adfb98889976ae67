"""cssm_fleet_smooth (include/cssm_pf.h; an EXTENSION): forward filtering, backward simulation of every series of a fleet.  Against the
sequential twin of the contract's backward simulation (tests/cpp/backsim_twin.c) run on the ORACLE's history -- the clouds and
ancestors of the CPU oracle stepping through the series, the records of cssm_fleet_pack_record:

  * traj_out bit for bit, ll_out bit for bit (the oracle's, which is cssm_fleet_interpolate's);
  * every order statistic bit for bit: the oracle's summary of the n_traj states the twin's trajectories name per time index;
  * the means (plain fp64 sums in another order) within rtol 1e-12 / atol 1e-13, the tolerance tests/test_gpu_fleet_interpolate.py
    holds the same sums to.

Sizes: N around the wave width, a non-power of two and CSSM_FLEET_MAX_N; n_traj 1, one group of 64, N and a value that does not divide
N.  The gathered cloud of a time index is staged in LDS up to 144 KiB (d N 8 bytes; beyond 48 KiB the launch asks for it by name):
d = 3 and d = 4 at N = 4096 run the large staging, d = 5 at N = 4096 (160 KiB) the L2 path by itself, and CSSM_OPT_SMOOTH_STAGING forces
the L2 path on shapes that would be staged."""
import numpy as np
import pytest

import cases
from composablestatespacemodels_amd import CssmError, Data, _abi
from composablestatespacemodels_amd.filter import FilterFleet, NativeLgcpFleet, NativePfFleet, Resampling
from oracle import oracle
from test_fleet_smooth_host import kinds_of, oracle_history, pack_records, twin_traj

pytestmark = pytest.mark.gpu
SEED = cases.SEED
NONE = 0xffffffff


def expected(model, n, seed, data, M, interval=0.975):
    """(ll, traj[T + 1, M], (mean, lower, upper, eta_of_mean, eta_lower, eta_upper)) of one series from the oracle and the twin"""
    t, y, has = data
    ll, X, Anc = oracle_history(model, n, seed, data)
    traj = twin_traj(X, Anc, pack_records(model, n, seed, t, y, has), kinds_of(model), seed, M)
    o = oracle.OraclePf(model.descriptor(), M, seed)
    times = np.concatenate([[np.min(t)], t])
    rows = []
    for s in range(len(t) + 1):
        o.init(float(times[s]))
        o.set_particles(X[s][:, traj[s]])
        rows.append(o.summary(interval))
    return ll, traj, tuple(np.array([r[q] for r in rows]) for q in range(6))


def assert_series(got_ll, got_rows, got_traj, want):
    ll, traj, (m, lo, hi, em, el, eu) = want
    assert got_ll == ll, (got_ll, ll)
    if got_traj is not None:
        np.testing.assert_array_equal(got_traj, traj)
    np.testing.assert_array_equal(got_rows[1], lo)
    np.testing.assert_array_equal(got_rows[2], hi)
    np.testing.assert_array_equal(got_rows[4], el)
    np.testing.assert_array_equal(got_rows[5], eu)
    np.testing.assert_allclose(got_rows[0], m, rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(got_rows[3], em, rtol=1e-12, atol=1e-13)
    assert np.all(np.isfinite(got_rows[0])) and np.all(np.isfinite(got_rows[5]))


def with_gap(data, lo, hi):
    t, y, has = data
    has = has.copy(); has[lo:hi] = 0
    return t, y, has


def off_divisor(n):
    """a trajectory count that does not divide n"""
    return next(m for m in (37, 41, 43) if n % m)


# 1 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [63, 64, 65, 1000, _abi.FLEET_MAX_N])
def test_one_component_every_size_and_trajectory_count(n):
    """c1, d = 1.  The records at t[0] = t0 have dt = 0 (the genealogical step); a removed observation leaves the identity behind it."""
    model = cases.c1_model()
    lengths = (2, 1, 1) if n == _abi.FLEET_MAX_N else (6, 1, 4)              # (the twin is sequential: N x n_traj x T evaluations)
    S = len(lengths)
    seeds = [SEED + 17 * k for k in range(S)]
    datas = [cases.poisson_counts(T, seed=SEED + k) for k, T in enumerate(lengths)]
    datas[0] = with_gap(datas[0], 1, 2)
    with NativePfFleet(model, n, S) as fl:
        fl.reseed(seeds)
        for M in (1, 64, n, off_divisor(n)):
            ll, rows, rc, traj = fl.smooth(datas, n_traj=M, want_trajectories=True)
            assert not rc.any(), rc
            for k in range(S):
                assert traj[k].shape == (lengths[k] + 1, M) and rows[k][0].shape == (lengths[k] + 1, 1)
                assert_series(ll[k], rows[k], traj[k], expected(model, n, seeds[k], datas[k], M))
        ms = fl.smooth_last_ms()
        assert len(ms) == 3 and all(v >= 0.0 for v in ms)


# 2 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,M", [(65, 65), (1000, 64), (1000, 37), (_abi.FLEET_MAX_N, 64)])
def test_three_components(n, M):
    """c2, d = 3 (OU components, a seasonal f): at N = 4096 the block stages 96 KiB."""
    model = cases.c2_model()
    lengths = (3, 1) if n == _abi.FLEET_MAX_N else (7, 2)
    seeds = [SEED + 17 * k for k in range(2)]
    datas = [cases.poisson_counts(T, seed=SEED + k, dt=0.5) for k, T in enumerate(lengths)]
    with NativePfFleet(model, n, 2) as fl:
        fl.reseed(seeds)
        ll, rows, rc, traj = fl.smooth(datas, n_traj=M, want_trajectories=True)
        assert not rc.any(), rc
        for k in range(2):
            assert_series(ll[k], rows[k], traj[k], expected(model, n, seeds[k], datas[k], M))


@pytest.mark.parametrize("d", list(range(1, 17)))
def test_every_latent_dimension(d):
    """One instantiation of each of the two kernels per latent dimension (tests/test_fleet_smooth_host.py holds this list to the source)."""
    model = cases.dim_model(d)
    S, n, M = 2, 257, 64
    seeds = [SEED + 17 * k for k in range(S)]
    datas = [with_gap(cases.poisson_counts(5, seed=SEED + k), 2, 3) for k in range(S)]
    with NativePfFleet(model, n, S) as fl:
        assert fl.d == d
        fl.reseed(seeds)
        ll, rows, rc, traj = fl.smooth(datas, n_traj=M, want_trajectories=True)
        assert not rc.any(), rc
        for k in range(S):
            assert_series(ll[k], rows[k], traj[k], expected(model, n, seeds[k], datas[k], M))


@pytest.mark.parametrize("d", [4, 5])
def test_the_threshold_between_staging_and_l2_at_the_largest_cloud(d):
    """N = 4096: d = 4 is the largest cloud a block stages (128 KiB of the 144 KiB it may ask for), d = 5 (160 KiB) goes through L2; either
    way forcing the L2 path changes nothing."""
    model = cases.dim_model(d)
    n, M = _abi.FLEET_MAX_N, 64
    seeds = [SEED + 17 * k for k in range(2)]
    datas = [cases.poisson_counts(T, seed=SEED + k) for k, T in enumerate((3, 2))]
    with NativePfFleet(model, n, 2) as fl:
        fl.reseed(seeds)
        got = fl.smooth(datas, n_traj=M, want_trajectories=True)
        assert not got[2].any()
        for k in range(2):
            assert_series(got[0][k], got[1][k], got[3][k], expected(model, n, seeds[k], datas[k], M))
        fl.set_option(_abi.CSSM_OPT_SMOOTH_STAGING, 1)
        _same(fl.smooth(datas, n_traj=M, want_trajectories=True), got)


def test_an_euler_affine_component():
    model = cases.euler_model()
    n, M, S = 257, 100, 2
    seeds = [SEED + 17 * k for k in range(S)]
    datas = [cases.poisson_counts(5 + k, seed=SEED + k, dt=0.25) for k in range(S)]
    assert list(kinds_of(model)) == [3, 3]
    with NativePfFleet(model, n, S) as fl:
        fl.reseed(seeds)
        ll, rows, rc, traj = fl.smooth(datas, n_traj=M, want_trajectories=True)
        assert not rc.any(), rc
        for k in range(S):
            assert_series(ll[k], rows[k], traj[k], expected(model, n, seeds[k], datas[k], M))


# 3 ------------------------------------------------------------------------------------------------------------------------------
def test_ragged_series_none_records_repeated_times_and_no_records():
    model = cases.c2_model()
    n, M = 300, 50
    t, y, has = cases.poisson_counts(9, seed=SEED)
    none_seen = (t, y, np.zeros(9, dtype=np.uint8))
    one = (np.array([2.5]), np.array([3.0]), np.ones(1, dtype=np.uint8))
    empty = (np.zeros(0), np.zeros(0), np.zeros(0, dtype=np.uint8))
    t2, y2, has2 = cases.poisson_counts(11, seed=SEED + 3, missing=0.3)
    t2 = t2.copy(); t2[5] = t2[4]; t2[8] = t2[7]               # repeated times inside the series: dt = 0, the genealogy
    has2 = has2.copy(); has2[5] = 1
    datas = [none_seen, one, empty, (t2, y2, has2)]
    S = len(datas)
    seeds = [SEED + 17 * k for k in range(S)]
    with NativePfFleet(model, n, S) as fl:
        fl.reseed(seeds)
        ll, rows, rc, traj = fl.smooth(datas, n_traj=M, want_trajectories=True)
        assert list(rc) == [0, 0, _abi.CSSM_EINVAL_ARG, 0]
        assert ll[0] == 0.0                                    # nothing was weighed
        for k in (0, 1, 3):
            assert_series(ll[k], rows[k], traj[k], expected(model, n, seeds[k], datas[k], M))
        assert np.isnan(ll[2]) and rows[2][0].shape == (1, 3) and all(np.all(np.isnan(a)) for a in rows[2])
        assert traj[2].shape == (1, M) and np.all(traj[2] == NONE)
        # the genealogical rows of series 3: the particle at index s is the parent of the particle at s + 1
        _, _, Anc = oracle_history(model, n, seeds[3], datas[3])
        for s in (0, 5, 8):                                    # record s has dt = 0 (record 0: t[0] is the series' t0)
            np.testing.assert_array_equal(traj[3][s], Anc[s][traj[3][s + 1]])
        # without the trajectories the rows are the same
        ll2, rows2, rc2 = fl.smooth(datas, n_traj=M)
        np.testing.assert_array_equal(ll2, ll)
        for k in range(S):
            for a, b in zip(rows2[k], rows[k]):
                np.testing.assert_array_equal(a, b)


def test_one_series_fails_and_the_others_do_not_notice():
    model = cases.linear_model()
    n, M, S = 1000, 200, 4
    seeds = [SEED + 17 * k for k in range(S)]
    datas = [cases.gaussian_series(8, seed=SEED + k) for k in range(S)]
    bad = datas[2][1].copy(); bad[3] = 1e200
    datas[2] = (datas[2][0], bad, datas[2][2])
    with pytest.raises(oracle.OracleError):                    # the premise: the oracle cannot filter that series either
        oracle_history(model, n, seeds[2], datas[2])
    with NativePfFleet(model, n, S) as fl:
        fl.reseed(seeds)
        ll, rows, rc, traj = fl.smooth(datas, n_traj=M, want_trajectories=True)
        assert list(rc) == [0, 0, _abi.CSSM_ENONFINITE, 0]
        assert np.isnan(ll[2]) and rows[2][0].shape == (9, 1) and all(np.all(np.isnan(a)) for a in rows[2]) and np.all(traj[2] == NONE)
        for k in (0, 1, 3):
            assert_series(ll[k], rows[k], traj[k], expected(model, n, seeds[k], datas[k], M))


# 4 ------------------------------------------------------------------------------------------------------------------------------
def _same(a, b):
    np.testing.assert_array_equal(a[0], b[0]); np.testing.assert_array_equal(a[2], b[2])
    for k in range(len(a[1])):
        for x, y in zip(a[1][k], b[1][k]):
            np.testing.assert_array_equal(x, y)
        np.testing.assert_array_equal(a[3][k], b[3][k])


def test_staging_and_chunks_change_nothing_and_ll_is_interpolates():
    S, n, M = 12, 1000, 100
    um = cases.c2_unparam()
    models = [um.run(cases.c2_params()) for _ in range(S)]
    seeds = [SEED + 17 * k for k in range(S)]
    datas = [with_gap(cases.poisson_counts(5 + (7 * k) % 11, seed=SEED + k, dt=(1, .5, .25)[k % 3]), 2, 3) for k in range(S)]
    per_series = [(len(d[0]) + 1) * n * (8 * 3 + 4) for d in datas]
    with NativePfFleet(models[0], n, S) as fl:
        fl.set_params(models); fl.reseed(seeds)
        whole = fl.smooth(datas, n_traj=M, want_trajectories=True)                # d N 8 = 24 KiB: staged in LDS
        assert not whole[2].any()
        assert_series(whole[0][5], whole[1][5], whole[3][5], expected(models[5], n, seeds[5], datas[5], M))
        fl.set_option(_abi.CSSM_OPT_SMOOTH_STAGING, 1)                            # the same call through L2
        _same(fl.smooth(datas, n_traj=M, want_trajectories=True), whole)
        fl.set_option(_abi.CSSM_OPT_SMOOTH_STAGING, 0)
        with pytest.raises(CssmError) as e:
            fl.set_option(_abi.CSSM_OPT_SMOOTH_STAGING, 2)
        assert e.value.code == _abi.CSSM_EINVAL_ARG
        big = max(per_series)
        for cap_kib in (-(-big // 1024), big // 2048):                            # one or two series per chunk; then every long one alone
            fl.set_option(_abi.CSSM_OPT_INTERP_CAP, cap_kib)
            _same(fl.smooth(datas, n_traj=M, want_trajectories=True), whole)
        fl.set_option(_abi.CSSM_OPT_INTERP_CAP, 0)
        ll, _, rc = fl.interpolate(datas)
        assert not rc.any()
        np.testing.assert_array_equal(ll, whole[0])


def test_the_fleet_and_an_open_window_are_untouched():
    S, n = 5, 500
    model = cases.c2_model()
    seeds = [SEED + 17 * k for k in range(S)]
    data_a = [cases.poisson_counts(6 + k, seed=SEED + k) for k in range(S)]
    data_b = [with_gap(cases.poisson_counts(9 + k, seed=SEED + 50 + k, dt=0.5), 3, 5) for k in range(S)]
    step_t = [np.array([float(d[0][-1]) + 0.5 * (q + 1) for d in data_a]) for q in range(3)]
    step_y = [np.arange(S, dtype=np.float64) + q for q in range(3)]
    with NativePfFleet(model, n, S) as fl, NativePfFleet(model, n, S) as twin:
        for f in (fl, twin):
            f.reseed(seeds)
            _, _, _, rc = f.ll_filter(data_a)
            assert not rc.any()
            f.window(4)
            f.step_interpolate(step_t[0], step_y[0], max_lag=2)
            f.step_interpolate(step_t[1], step_y[1], max_lag=2)
        before = [(fl.particles(k), fl.ancestors(k), fl.observation_index(k), fl.window_depth(k)) for k in range(S)], fl.summary()
        with pytest.raises(CssmError) as e:
            fl.smooth_last_ms()
        assert e.value.code == _abi.CSSM_ESTATE
        ll, rows, rc = fl.smooth(data_b, n_traj=64)
        assert not rc.any()
        assert_series(ll[1], rows[1], None, expected(model, n, seeds[1], data_b[1], 64))
        after = [(fl.particles(k), fl.ancestors(k), fl.observation_index(k), fl.window_depth(k)) for k in range(S)], fl.summary()
        for (pa, aa, ia, wa), (pb, ab, ib, wb) in zip(before[0], after[0]):
            np.testing.assert_array_equal(pa, pb); np.testing.assert_array_equal(aa, ab)
            assert ia == ib and wa == wb == 2
        for x, y in zip(before[1], after[1]):
            np.testing.assert_array_equal(x, y)
        got, want = fl.step_interpolate(step_t[2], step_y[2], max_lag=2), twin.step_interpolate(step_t[2], step_y[2], max_lag=2)
        for x, y in zip((got[0], got[1], got[2], *got[3], got[4]), (want[0], want[1], want[2], *want[3], want[4])):
            np.testing.assert_array_equal(x, y)                # ll, ess, rows_out, the window's rows (the lineages reach behind the call), rc
    with NativePfFleet(model, n, S) as fl:                     # a fleet that was never initialised serves the call, and is no more initialised for it
        fl.reseed(seeds)
        ll, rows, rc = fl.smooth(data_b, n_traj=64)
        assert not rc.any()
        with pytest.raises(CssmError) as e:
            fl.step(step_t[0], step_y[0])
        assert e.value.code == _abi.CSSM_ESTATE and fl.observation_index(0) == 0


# 5 ------------------------------------------------------------------------------------------------------------------------------
def test_refusals_that_need_a_fleet_name_the_call():
    t, y, has = cases.event_times(5)
    with NativeLgcpFleet(cases.c4_model(), 100, 2, 2) as fl:
        with pytest.raises(CssmError, match="cssm_fleet_smooth: an LGCP fleet") as e:
            fl.smooth([(t, y, has)] * 2)
        assert e.value.code == _abi.CSSM_EINVAL_ARG and "chain of sub-steps" in str(e.value)
    model = cases.c1_model()
    datas = [cases.poisson_counts(3, seed=SEED + k) for k in range(2)]
    with NativePfFleet(model, 100, 2) as fl:
        off, tt, yy, hh = fl.pack(datas)
        ll, rc = np.zeros(2), np.zeros(2, dtype=np.int32)
        import ctypes as C
        p = lambda a, ty: a.ctypes.data_as(C.POINTER(ty))
        code = fl.lib.cssm_fleet_smooth(fl._h, p(off, C.c_uint64), p(tt, C.c_double), p(yy, C.c_double), p(hh, C.c_uint8), 10, 0.975,
                                        _abi.CSSM_INTERP_REFERENCE_PAIRING, p(ll, C.c_double), *([None] * 6), None, p(rc, C.c_int))
        msg = fl.lib.cssm_last_error()
        assert code == _abi.CSSM_EINVAL_ARG and b"cssm_fleet_smooth" in msg and b"CSSM_INTERP_REFERENCE_PAIRING" in msg
        bad = off.copy(); bad[1] = 7                           # a decreasing off is seen once S is known
        code = fl.lib.cssm_fleet_smooth(fl._h, p(bad, C.c_uint64), p(tt, C.c_double), p(yy, C.c_double), p(hh, C.c_uint8), 10, 0.975, 0,
                                        p(ll, C.c_double), *([None] * 6), None, p(rc, C.c_int))
        assert code == _abi.CSSM_EINVAL_ARG and b"non-decreasing" in fl.lib.cssm_last_error()


def test_filter_fleet_in_the_reference_vocabulary():
    S, n = 2, 300
    um = cases.c2_unparam()
    models = [um.run(cases.c2_params()) for _ in range(S)]
    datas = []
    for k in range(S):
        t, y, has = with_gap(cases.poisson_counts(6 + 2 * k, seed=SEED + k, missing=0.2), 2, 4)
        datas.append([Data(float(a), float(b) if h else None) for a, b, h in zip(t, y, has)])
    with FilterFleet(models, Resampling.systematicResampling, n, seed=SEED) as ff:
        outs = ff.smooth(datas, n_traj=100, interval=0.9)
        inter = ff.interpolate(datas, 0.9)
        assert len(outs) == S
        for k in range(S):
            assert outs[k][0] == inter[k][0] and len(outs[k][1]) == len(datas[k]) + 1
            assert [o.time for o in outs[k][1]] == [o.time for o in inter[k][1]]
            assert [o.observation for o in outs[k][1]] == [o.observation for o in inter[k][1]]
            assert all(np.all(np.isfinite(o.state)) and o.stateIntervals[0].lower <= o.stateIntervals[0].upper for o in outs[k][1])
        ms = ff.smooth_last_ms()
        assert len(ms) == 3 and all(v >= 0.0 for v in ms)
