"""cssm_pf_window / cssm_pf_step_interpolate (include/cssm_pf.h; csrc/cssm_intervals.hip: k_lineage_fill, k_slice_put): the fixed-lag
interpolation of ONE live cloud.  The reference of every row is the only route the library had before: cssm_pf_interpolate over the
prefix of the records on another handle -- bit for bit, order statistics AND means --, the filter's own results are cssm_pf_step's on a
twin handle, and for the small clouds the oracle's interpolate (ll and order statistics exact, the means -- plain fp64 sums in another
order -- within rtol 1e-12 / atol 1e-13, the tolerance of tests/test_interpolate.py for the same sums).

A lag >= slices is refused by contract (CSSM_EINVAL_ARG naming both numbers): where the lags of a stream cycle beyond the ring, the
test holds the call to that refusal, sees the handle and the window untouched, and makes the record's call with lag = slices - 1 -- which
still reaches beyond the depth while the window fills."""
import ctypes as C
import math

import numpy as np
import pytest

import cases
from composablestatespacemodels_amd import CssmError, Data, _abi
from composablestatespacemodels_amd.filter import FilterInterpolate, NativePf, Resampling
from test_filter_intervals_host import exact_order_statistics
from test_gpu_fleet_interpolate import oracle_interpolate, with_gap

pytestmark = pytest.mark.gpu
SEED = cases.SEED
ROW_NAMES = ("state_mean", "state_lower", "state_upper", "eta_of_mean", "eta_lower", "eta_upper")
_dp = C.POINTER(C.c_double)


def prefix_of(data, m):
    """records 0 .. m"""
    return tuple(a[:m + 1] for a in data)


def same_tail(rows, nrows, want, m, what="", depth=None):
    """Row j of ``rows`` (the six arrays of a step_interpolate call behind record m) against row m + 1 - j of ``want`` = the six arrays
    of the prefix interpolation; rows from ``nrows`` on read NaN."""
    for q, name in enumerate(ROW_NAMES):
        got = rows[q]
        for j in range(nrows):
            np.testing.assert_array_equal(got[j], want[q][m + 1 - j], err_msg=f"{what} record {m} row {j} {name}")
        assert np.isnan(got[nrows:]).all(), (what, m, name)


def close_to_oracle(rows, nrows, ll, want, m, what=""):
    """... against the oracle's interpolate of the prefix: (ll, mean, lower, upper, eta_of_mean, eta_lower, eta_upper)"""
    assert ll == want[0], (what, m)
    for q, name in enumerate(ROW_NAMES):
        for j in range(nrows):
            if name in ("state_mean", "eta_of_mean"):
                np.testing.assert_allclose(rows[q][j], want[1 + q][m + 1 - j], rtol=1e-12, atol=1e-13, err_msg=f"{what} record {m} row {j} {name}")
            else:
                np.testing.assert_array_equal(rows[q][j], want[1 + q][m + 1 - j], err_msg=f"{what} record {m} row {j} {name}")


def refused(g: NativePf, t, y, lag, interval=0.975):
    """(code, message) of a step_interpolate the library refuses"""
    with pytest.raises(CssmError) as e:
        g.step_interpolate(t, y, lag=lag, interval=interval)
    return e.value.code, str(e.value)


def stream_against_prefixes(model, n, data, slices, lags, option=None, oracle_too=False, what=""):
    """Drive handle a through the records with step_interpolate (window of ``slices``, lag of record m = lags[m % len(lags)]), a twin b
    with step, and hold every call to the prefix interpolation on a third handle c."""
    t, y, has = data
    t0 = float(np.min(t))
    with NativePf(model, n, SEED) as a, NativePf(model, n, SEED) as b, NativePf(model, n, SEED) as c:
        if option is not None:
            for g in (a, b, c):
                g.set_option(*option)
        a.init(t0); b.init(t0)
        a.window(slices)
        assert a.window_depth() == 0
        for m in range(len(t)):
            lag = lags[m % len(lags)]
            if lag >= slices:
                depth, idx = a.window_depth(), a.observation_index()
                code, msg = refused(a, float(t[m]), float(y[m]) if has[m] else None, lag)
                assert code == _abi.CSSM_EINVAL_ARG and str(lag) in msg and str(slices) in msg, msg
                assert a.window_depth() == depth and a.observation_index() == idx
                lag = slices - 1
            ll, ess, nrows, rows = a.step_interpolate(float(t[m]), float(y[m]), bool(has[m]), lag=lag)
            assert (ll, ess) == b.step(float(t[m]), float(y[m]), bool(has[m])), (what, m)
            depth = min(m + 1, slices - 1)
            assert a.window_depth() == depth and nrows == min(lag, depth) + 1, (what, m, a.window_depth(), nrows)
            assert rows[0].shape == (lag + 1, a.d) and rows[3].shape == (lag + 1,)
            want = c.interpolate(*prefix_of(data, m))
            assert ll == want[0], (what, m)
            same_tail(rows, nrows, want[1:], m, what)
            if oracle_too:
                close_to_oracle(rows, nrows, ll, oracle_interpolate(model, n, SEED, prefix_of(data, m)), m, what)


# 1 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 1000, 4097, 70001, 300001])   # 4097: across CSSM_IV_CAP; 70001: cand_max > CSSM_IV_CAP; 300001: the grid-stride loops run
def test_every_prefix(n):
    T = 5 if n == 300001 else 8
    data = with_gap(cases.poisson_counts(T), 2, 4)
    stream_against_prefixes(cases.c2_model(), n, data, 4, list(range(6)), oracle_too=n <= 4097, what=f"n={n}")


# 2 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", list(range(1, 17)))
def test_every_latent_dimension(d):
    model = cases.dim_model(d)
    data = with_gap(cases.poisson_counts(6), 2, 4)
    stream_against_prefixes(model, 257, data, 3, [2], oracle_too=True, what=f"d={d}")


# 3 ------------------------------------------------------------------------------------------------------------------------------
def same_handles(a: NativePf, b: NativePf, what=""):
    np.testing.assert_array_equal(a.particles(), b.particles(), err_msg=f"{what} particles")
    np.testing.assert_array_equal(a.ancestors(), b.ancestors(), err_msg=f"{what} ancestors")
    assert a.observation_index() == b.observation_index(), what


def test_the_handle_is_left_as_step_leaves_it():
    model, n = cases.c2_model(), 1000
    t, y, has = with_gap(cases.poisson_counts(8), 2, 4)
    with NativePf(model, n, SEED) as a, NativePf(model, n, SEED) as b:
        a.init(0.0); b.init(0.0)
        a.window(4)
        for m in range(len(t)):
            ll, ess, nrows, rows = a.step_interpolate(float(t[m]), float(y[m]), bool(has[m]), lag=m % 4)
            r = b.step_intervals(float(t[m]), float(y[m]), bool(has[m]))
            assert (ll, ess) == (r[0], r[1]), m
            same_handles(a, b, f"record {m}")
            for q, name in enumerate(ROW_NAMES):                                # row 0: the summary behind the step
                np.testing.assert_array_equal(rows[q][0], r[2 + q], err_msg=f"record {m} {name}")
        # the clock, the level state and the sums state show in what follows: a step, then a continued batch call
        tn = float(t[-1])
        assert a.step(tn + 1.0, 2.0) == b.step(tn + 1.0, 2.0)
        same_handles(a, b, "one more step")
        t2, y2, h2 = np.array([tn + 2.0, tn + 2.5, tn + 4.0]), np.array([1.0, 0.0, 3.0]), np.array([1, 0, 1], dtype=np.uint8)
        ra, rb = a.run_more(t2, y2, h2), b.run_more(t2, y2, h2)
        assert ra[0] == rb[0]
        np.testing.assert_array_equal(ra[1], rb[1]); np.testing.assert_array_equal(ra[2], rb[2])
        same_handles(a, b, "a continued call")


# 4 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("resampler", [1, 2])                                # stratified; multinomial (ancestors not sorted: the other gather pattern)
def test_stratified_and_multinomial_resamplers(resampler):
    data = with_gap(cases.poisson_counts(8), 2, 4)
    stream_against_prefixes(cases.c2_model(), 1000, data, 4, [3, 1, 2], option=(2, resampler), what=f"resampler {resampler}")   # CSSM_OPT_RESAMPLER


# 5 ------------------------------------------------------------------------------------------------------------------------------
def test_a_held_and_redone_observation_inside_the_stream():
    """The outlier of test_gpu_filter_intervals.test_a_held_and_redone_observation: the step is put on hold at record 5 and redone; the
    slice and the rows behind the hold returned at once and are enqueued again behind the redo."""
    t, y, has = cases.poisson_counts(9, missing=0.2)
    y = y.copy(); y[5] = 70.0; has = has.copy(); has[5] = 1
    stream_against_prefixes(cases.c2_model(), 4096, (t, y, has), 5, [4, 2], what="held")


# 6 ------------------------------------------------------------------------------------------------------------------------------
def _pmmh(g: NativePf, t, y, has):
    model = cases.c2_model()
    theta0 = np.ascontiguousarray(cases.c2_params().flattenParams(), dtype=np.float64)
    iters = 2
    ll = np.zeros(iters); th = np.zeros((iters, theta0.size)); acc = np.zeros(iters, dtype=np.int32); last = np.zeros((iters, g.d))
    hh = np.ascontiguousarray(has, dtype=np.uint8)
    desc = model.descriptor()
    _abi.check(g.lib.cssm_pmmh_run(g._h, desc.ptr(), theta0.ctypes.data_as(_dp), theta0.size, 0.0025, t.ctypes.data_as(_dp),
                                   y.ctypes.data_as(_dp), hh.ctypes.data_as(C.POINTER(C.c_uint8)), len(t), SEED, iters, ll.ctypes.data_as(_dp),
                                   th.ctypes.data_as(_dp), acc.ctypes.data_as(C.POINTER(C.c_int32)), last.ctypes.data_as(_dp)))
    g.generation += 1


def _propagate_adopt(g: NativePf, t):
    g.propagate(t, 2.0)
    g.adopt(g.proposed(), -1.5, g.n // 2)


T3, Y3, H3 = np.array([3.0, 3.5, 4.0]), np.array([1.0, 2.0, 0.0]), np.array([1, 0, 1], dtype=np.uint8)
# the calls that write the handle's cloud, key or parameters: (name, the call, whether the handle needs a new cloud afterwards)
RESTARTS = [
    ("init", lambda g: g.init(3.0), False),
    ("init_from", lambda g: g.init_from(3.0, [0.1, 0.2, 0.3]), False),
    ("step", lambda g: g.step(3.0, 2.0), False),
    ("step_intervals", lambda g: g.step_intervals(3.0, 2.0), False),
    ("step_forecast", lambda g: g.step_forecast(3.0, 2.0), False),
    ("propagate, adopt", lambda g: _propagate_adopt(g, 3.0), False),
    ("adopt", lambda g: g.adopt(g.particles(), -1.0, 7), False),
    ("ll_filter", lambda g: g.run(T3, Y3, H3), False),
    ("ll_filter_more", lambda g: g.run_more(T3, Y3, H3), False),
    ("filter", lambda g: g.run(T3, Y3, H3, want_path=True), False),
    ("filter_intervals", lambda g: g.filter_intervals(T3, Y3, H3), False),
    ("filter_intervals_more", lambda g: g.filter_intervals_more(T3, Y3, H3), False),
    ("filter_forecasts", lambda g: g.filter_forecasts(T3, Y3, H3), False),
    ("filter_forecasts_more", lambda g: g.filter_forecasts_more(T3, Y3, H3), False),
    ("interpolate", lambda g: g.interpolate(T3, Y3, H3), True),
    ("smooth", lambda g: g.smooth(T3, Y3, H3, n_traj=64), True),
    ("pmmh_run", lambda g: _pmmh(g, T3, Y3, H3), False),
    ("reseed", lambda g: g.reseed(SEED + 5), False),
    ("set_params", lambda g: g.set_params(cases.c2_model()), False),
    ("set_option(CSSM_OPT_RESAMPLER)", lambda g: g.set_option(2, 1), False),
]


@pytest.mark.parametrize("name", [r[0] for r in RESTARTS])
def test_every_call_that_writes_the_handle_restarts_the_window(name):
    _, call, reinit = next(r for r in RESTARTS if r[0] == name)
    model, n = cases.c2_model(), 500
    with NativePf(model, n, SEED) as a, NativePf(model, n, SEED) as b:
        a.init(0.0); b.init(0.0)
        a.window(4)
        for tt, yy in ((1.0, 2.0), (2.0, 1.0)):
            assert a.step_interpolate(tt, yy, lag=3)[:2] == b.step(tt, yy)
        assert a.window_depth() == 2
        call(a); call(b)
        assert a.window_depth() == 0, name
        if reinit:
            a.init(4.0); b.init(4.0)
            assert a.window_depth() == 0
        ll, ess, nrows, rows = a.step_interpolate(5.0, 3.0, lag=3)
        assert (ll, ess) == b.step(5.0, 3.0), name
        assert a.window_depth() == 1 and nrows == 2, (name, nrows)
        want = b.summary()
        for q, rn in enumerate(ROW_NAMES):
            np.testing.assert_array_equal(rows[q][0], want[q], err_msg=f"{name} {rn}")
            assert np.isfinite(rows[q][1]).all() and np.isnan(rows[q][2:]).all(), (name, rn)
        same_handles(a, b, name)


def test_rows_behind_a_restart_by_step_are_the_prefix_interpolation_s_to_the_base_slice():
    model, n = cases.c2_model(), 1000
    data = with_gap(cases.poisson_counts(8), 2, 4)
    t, y, has = data
    restart_at = 3                                                            # record a = 3 is made by cssm_pf_step
    with NativePf(model, n, SEED) as a, NativePf(model, n, SEED) as c:
        a.init(float(np.min(t)))
        a.window(6)
        for m in range(len(t)):
            if m == restart_at:
                a.step(float(t[m]), float(y[m]), bool(has[m]))
                assert a.window_depth() == 0
                continue
            ll, ess, nrows, rows = a.step_interpolate(float(t[m]), float(y[m]), bool(has[m]), lag=5)
            depth = m + 1 if m < restart_at else m - restart_at
            assert a.window_depth() == depth and nrows == depth + 1, (m, a.window_depth(), nrows)
            same_tail(rows, nrows, c.interpolate(*prefix_of(data, m))[1:], m, "behind a restart")


def test_reading_calls_leave_the_window_alone_and_windows_open_and_close():
    model, n = cases.c2_model(), 1000
    data = with_gap(cases.poisson_counts(8), 2, 4)
    t, y, has = data
    with NativePf(model, n, SEED) as a, NativePf(model, n, SEED) as c, NativePf(model, n, SEED) as plain:
        a.init(float(np.min(t))); plain.init(float(np.min(t)))
        a.window(4)
        for m in range(5):
            a.summary(); a.forecast([float(t[m]) + 0.25]); a.particles(); a.ancestors(); a.proposed()
            depth = a.window_depth()
            ll, ess, nrows, rows = a.step_interpolate(float(t[m]), float(y[m]), bool(has[m]), lag=3)
            assert (ll, ess) == plain.step(float(t[m]), float(y[m]), bool(has[m]))      # a handle that never opened a window: the same bits
            assert a.window_depth() == min(depth + 1, 3) == min(m + 1, 3)
            same_tail(rows, nrows, c.interpolate(*prefix_of(data, m))[1:], m, "reads in between")
        a.window(0)
        assert a.window_depth() == 0
        code, msg = refused(a, float(t[5]), 1.0, 2)
        assert code == _abi.CSSM_ESTATE and "cssm_pf_window" in msg
        a.window(7)                                                           # another size: the window starts again from the cloud the handle holds
        assert a.window_depth() == 0
        ll, ess, nrows, rows = a.step_interpolate(float(t[5]), float(y[5]), bool(has[5]), lag=6)
        assert (ll, ess) == plain.step(float(t[5]), float(y[5]), bool(has[5])) and a.window_depth() == 1 and nrows == 2
        a.window(7)                                                           # re-opening restarts
        assert a.window_depth() == 0
        assert a.step_interpolate(float(t[6]), float(y[6]), bool(has[6]), lag=None)[:3] == plain.step(float(t[6]), float(y[6]), bool(has[6])) + (0,)
        assert a.window_depth() == 1
        np.testing.assert_array_equal(a.particles(), plain.particles())


# 7 ------------------------------------------------------------------------------------------------------------------------------
def test_interleaving_with_the_filtered_intervals_on_one_handle():
    """step_interpolate, step_intervals and filter_intervals_more on one handle, each on a scratch of its own: every call's rows are
    right.  (The calls in between restart the window: row 0 of the next step_interpolate is the summary behind it, row 1 the base slice --
    the cloud before it -- through the ancestors of the step: its order statistics by a sort in numpy, its means within the bound of a sum
    in another order.)"""
    model, n = cases.c2_model(), 5000
    with NativePf(model, n, SEED) as a, NativePf(model, n, SEED) as b:
        a.init(0.0); b.init(0.0)
        a.window(3)
        tt = 0.0
        for rep in range(3):
            tt += 1.0
            assert a.step(tt, 1.0) == b.step(tt, 1.0) and a.window_depth() == 0    # (a plain step: the window starts again)
            cloud0 = b.particles()
            tt += 1.0
            ll, ess, nrows, rows = a.step_interpolate(tt, 2.0, lag=2)
            assert (ll, ess) == b.step(tt, 2.0) and nrows == 2
            after = b.summary()
            lineage = cloud0[:, b.ancestors()]                                # the base slice through the lineages that survive the step
            for q, rn in enumerate(ROW_NAMES):
                np.testing.assert_array_equal(rows[q][0], after[q], err_msg=f"rep {rep} {rn} row 0")
            for k in range(a.d):
                lohi = exact_order_statistics(lineage[k], 0.975, True)
                assert (rows[1][1, k], rows[2][1, k]) == (lohi[0], lohi[1]), (rep, k)
            np.testing.assert_allclose(rows[0][1], lineage.mean(axis=1), rtol=1e-12, atol=1e-13)
            tt += 1.0
            r = a.step_intervals(tt, 1.0)
            assert (r[0], r[1]) == b.step(tt, 1.0)
            want = b.summary()
            for q, rn in enumerate(ROW_NAMES):
                np.testing.assert_array_equal(r[2 + q], want[q], err_msg=f"rep {rep} step_intervals {rn}")
            t2, y2 = np.array([tt + 0.5, tt + 1.0]), np.array([0.0, 3.0])
            tt += 1.0
            got = a.filter_intervals_more(t2, y2)
            rows2 = []
            for s in range(2):
                b.step(float(t2[s]), float(y2[s])); rows2.append(b.summary())
            for q, rn in enumerate(ROW_NAMES):
                np.testing.assert_array_equal(got[3 + q], np.array([r2[q] for r2 in rows2]), err_msg=f"rep {rep} filter_intervals_more {rn}")
            # two consecutive calls: depth 2, three rows, the oldest still the base slice
            tt += 1.0
            a.step_interpolate(tt, 2.0, lag=None); b.step(tt, 2.0)
            tt += 1.0
            ll, ess, nrows, rows = a.step_interpolate(tt, 0.0, lag=2)
            assert (ll, ess) == b.step(tt, 0.0) and nrows == 3 and a.window_depth() == 2
            want = b.summary()
            for q, rn in enumerate(ROW_NAMES):
                np.testing.assert_array_equal(rows[q][0], want[q], err_msg=f"rep {rep} {rn}")
                assert np.isfinite(rows[q]).all()


# 8 ------------------------------------------------------------------------------------------------------------------------------
def test_step_interpolate_last_ms():
    with NativePf(cases.c2_model(), 70001, SEED) as g:
        g.init(0.0)
        g.window(4)
        with pytest.raises(CssmError) as e:
            g.step_interpolate_last_ms()
        assert e.value.code == _abi.CSSM_ESTATE
        g.step_interpolate(1.0, 2.0, lag=2)
        ms = g.step_interpolate_last_ms()
        assert all(math.isfinite(v) for v in ms) and ms[0] > 0.0 and ms[1] > 0.0, ms
        assert ms == g.step_interpolate_last_ms()
        g.step_interpolate(2.0, 1.0, lag=None)
        ms = g.step_interpolate_last_ms()
        assert all(math.isfinite(v) for v in ms) and ms[0] > 0.0 and ms[1] == 0.0, ms


# 9 ------------------------------------------------------------------------------------------------------------------------------
def test_refusals_by_code_and_message():
    lib = _abi.load_library()
    six = [None] * 6
    E, S, M = _abi.CSSM_EINVAL_ARG, _abi.CSSM_ESTATE, _abi.CSSM_ENOMEM
    with NativePf(cases.c2_model(), 1000, SEED) as g, NativePf(cases.c2_model(), 1000, SEED) as b:
        assert lib.cssm_pf_step_interpolate(g._h, 1.0, 1.0, 1, 0, 0.975, None, None, None, *six) == S and b"cssm_pf_window" in lib.cssm_last_error()
        assert lib.cssm_pf_window(g._h, 1) == E and b"2 slices" in lib.cssm_last_error()
        assert lib.cssm_pf_window(g._h, 4) == 0
        assert lib.cssm_pf_step_interpolate(g._h, 1.0, 1.0, 1, 0, 0.975, None, None, None, *six) == S and b"before cssm_pf_init" in lib.cssm_last_error()
        ms = np.full(2, 7.0)
        assert lib.cssm_pf_step_interpolate_last_ms(g._h, ms.ctypes.data_as(_dp)) == S and list(ms) == [7.0, 7.0]
        assert lib.cssm_pf_step_interpolate_last_ms(g._h, None) == E
        g.init(0.0); b.init(0.0)
        for bad in (0.0, 1.5, float("nan")):
            assert lib.cssm_pf_step_interpolate(g._h, 1.0, 1.0, 1, 0, bad, None, None, None, *six) == E and b"interval must be in (0, 1]" in lib.cssm_last_error()
        for lag in (4, 5, 0xFFFFFFFE):
            assert lib.cssm_pf_step_interpolate(g._h, 1.0, 1.0, 1, lag, 0.975, None, None, None, *six) == E
            assert str(lag).encode() in lib.cssm_last_error() and b"4" in lib.cssm_last_error()
        assert g.window_depth() == 0 and g.observation_index() == 0           # refused before any work
        # every output may be null
        assert lib.cssm_pf_step_interpolate(g._h, 1.0, 1.0, 1, 3, 0.975, None, None, None, *six) == 0
        assert b.step(1.0, 1.0) and g.window_depth() == 1
        # a window far beyond any device: CSSM_ENOMEM naming the bytes, nothing allocated, and the handle goes on without a window
        assert lib.cssm_pf_window(g._h, 1 << 31) == M
        msg = lib.cssm_last_error()
        assert b"bytes" in msg and str(1 << 31).encode() in msg, msg
        assert b"the device has" in msg, msg                                   # (the refusal made from the count alone, before any allocation)
        assert g.window_depth() == 0
        assert lib.cssm_pf_step_interpolate(g._h, 2.0, 1.0, 1, 0, 0.975, None, None, None, *six) == S and b"cssm_pf_window" in lib.cssm_last_error()
        assert lib.cssm_pf_window(g._h, 0xFFFFFFFF) == M                       # (the byte count itself is formed without overflow)
        assert g.step(2.0, 2.0) == b.step(2.0, 2.0)                            # the handle keeps streaming
        g.window(3)
        ll, ess, nrows, rows = g.step_interpolate(3.0, 1.0, lag=2)
        assert (ll, ess) == b.step(3.0, 1.0) and nrows == 2
        np.testing.assert_array_equal(g.particles(), b.particles())
    with NativePf(cases.c4_model(), 500, SEED, lgcp_precision=1) as g:        # an LGCP handle: cssm_pf_interpolate's refusal
        want = b"the LGCP filter has no path variant"
        assert lib.cssm_pf_window(g._h, 4) == E and want in lib.cssm_last_error()
        assert lib.cssm_pf_step_interpolate(g._h, 1.0, 1.0, 1, 0, 0.975, None, None, None, *six) == E and want in lib.cssm_last_error()
    h = C.c_void_p()                                                          # the only shard of a cloud of 1000, on the default stream
    _abi.check(lib.cssm_pf_create_shard(cases.c2_model().descriptor().ptr(), 1000, 0, 1000, SEED, 0, None, C.byref(h)))
    try:
        assert lib.cssm_pf_window(h, 4) == S and b"sharded handle" in lib.cssm_last_error()
        assert lib.cssm_pf_step_interpolate(h, 1.0, 1.0, 1, 0, 0.975, None, None, None, *six) == S and b"sharded handle" in lib.cssm_last_error()
    finally:
        lib.cssm_pf_destroy(h)


# 10 -----------------------------------------------------------------------------------------------------------------------------
def test_filter_interpolate_step_interpolate_gives_the_tail_of_interpolate():
    model, n = cases.c2_model(), 1000
    t, y, has = with_gap(cases.poisson_counts(8), 2, 4)
    data = [Data(float(a), float(b) if h else None) for a, b, h in zip(t, y, has)]
    flt = FilterInterpolate(model, Resampling.systematicResampling, seed=SEED)
    ref = FilterInterpolate(model, Resampling.systematicResampling, seed=SEED)
    s = flt.initialiseState(n, float(np.min(t)))
    flt.window(4)
    for m, dd in enumerate(data):
        s, outs = flt.stepInterpolate(s, dd, 3)
        ll, want = ref.interpolate(data[:m + 1], n)
        assert s.ll == ll and (s.t, s.observation) == (dd.t, dd.observation)
        assert len(outs) == min(3, m + 1) + 1
        for a, b in zip(outs, want[len(want) - len(outs):]):                  # oldest first, as interpolate returns them
            assert (a.time, a.observation, a.eta, a.etaIntervals, a.stateIntervals) == (b.time, b.observation, b.eta, b.etaIntervals, b.stateIntervals)
            np.testing.assert_array_equal(a.state, b.state)
    s, outs = flt.stepInterpolate(s, Data(float(t[-1]) + 1.0, 2.0), None)
    assert outs == []
