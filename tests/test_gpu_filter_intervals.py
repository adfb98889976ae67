"""cssm_pf_filter_intervals / _more / cssm_pf_step_intervals (include/cssm_pf.h; csrc/cssm_intervals.hip): the filtered intervals of one
cloud, a row per observation from the batch call.  The reference of every row is the route the library had before: cssm_pf_summary at
that moment of the loop init; summary; (step; summary)* on a second handle of the same seed -- bit for bit, order statistics AND means --,
and the filter's own results are cssm_pf_ll_filter's.  The selection is also held to a sort of the order keys in numpy and to its
sequential twin (tests/cpp/intervals_twin.c) on clouds that break a selection, put on the device through cssm_pf_adopt."""
import ctypes as C
import math

import numpy as np
import pytest

import cases
from composablestatespacemodels_amd import CssmError, Data, _abi
from composablestatespacemodels_amd.filter import Filter, NativePf, ParticleFilter, Resampling
from oracle import oracle
from test_filter_intervals_host import INTERVALS, SIZES, crafted_clouds, exact_order_statistics, ranks, twin_select

pytestmark = pytest.mark.gpu
SEED = cases.SEED
ROW_NAMES = ("state_mean", "state_lower", "state_upper", "eta_of_mean", "eta_lower", "eta_upper")


def series(T=12):
    """T = 12 Poisson counts, record 3 without a datum, records 6 and 7 at the same time (dt = 0)."""
    t, y, has = cases.poisson_counts(T)
    t, y, has = t.copy(), y.copy(), has.copy()
    has[3] = 0
    t[7] = t[6]
    return t, y, has


def loop_rows(g: NativePf, t, y, has, interval=0.975, init=True):
    """The route before this call existed: (ll, ll_t, ess_t, six row arrays) of init; summary; (step; summary)* on the handle g."""
    rows, ll_t, ess_t = [], [], []
    if init:
        g.init(float(np.min(t)))
        rows.append(g.summary(interval))
    for s in range(len(t)):
        ll, ess = g.step(float(t[s]), float(y[s]), bool(has[s]))
        ll_t.append(ll); ess_t.append(ess)
        rows.append(g.summary(interval))
    six = tuple(np.array([r[j] for r in rows]) for j in range(6))
    return (ll_t[-1], np.array(ll_t), np.array(ess_t, dtype=np.int32)) + six


def same_rows(got, want, what=""):
    assert got[0] == want[0], what
    np.testing.assert_array_equal(got[1], want[1], err_msg=f"{what} ll_t")
    np.testing.assert_array_equal(got[2], want[2], err_msg=f"{what} ess_t")
    for j, name in enumerate(ROW_NAMES):
        assert got[3 + j].shape == want[3 + j].shape, (what, name)
        np.testing.assert_array_equal(got[3 + j], want[3 + j], err_msg=f"{what} {name}")


def same_handles(a: NativePf, b: NativePf, t_next, what=""):
    """cloud and ancestors, then one further step on both routes (clock, observation index, LGCP level and sums state show there)"""
    np.testing.assert_array_equal(a.particles(), b.particles(), err_msg=f"{what} particles")
    np.testing.assert_array_equal(a.ancestors(), b.ancestors(), err_msg=f"{what} ancestors")
    assert a.observation_index() == b.observation_index(), what
    assert a.step(t_next, 2.0) == b.step(t_next, 2.0), what
    np.testing.assert_array_equal(a.particles(), b.particles(), err_msg=f"{what} particles after one more step")


def both_routes(model, n, t, y, has, interval=0.975, option=None, t_next=None, **kw):
    with NativePf(model, n, SEED, **kw) as a, NativePf(model, n, SEED, **kw) as b:
        if option is not None:
            a.set_option(*option); b.set_option(*option)
        got = a.filter_intervals(t, y, has, interval)
        want = loop_rows(b, t, y, has, interval)
        same_rows(got, want, f"n={n}")
        same_handles(a, b, float(t[-1]) + 1.0 if t_next is None else t_next, f"n={n}")
        return got


# 1 ------------------------------------------------------------------------------------------------------------------------------
MODELS = {"c1": cases.c1_model, "c2": cases.c2_model, "c3": cases.c3_model, "d16": lambda: cases.dim_model(16)}


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 1000, 4097, 300001])      # the last: more than 1024 x CSSM_BLOCK, the grid-stride loops run
@pytest.mark.parametrize("name", list(MODELS))
def test_rows_have_the_bits_of_the_step_and_summary_loop(name, n):
    t, y, has = series()
    got = both_routes(MODELS[name](), n, t, y, has)
    d = MODELS[name]().dimension
    assert got[3].shape == (13, d) and got[6].shape == (13,)
    with NativePf(MODELS[name](), n, SEED) as c:                               # the filter's results: cssm_pf_ll_filter's
        ll, ll_t, ess_t, _ = c.run(t, y, has)
    assert got[0] == ll
    np.testing.assert_array_equal(got[1], ll_t); np.testing.assert_array_equal(got[2], ess_t)


# 2 ------------------------------------------------------------------------------------------------------------------------------
def test_rows_against_the_oracle_s_summary_chain():
    model, n = cases.c2_model(), 500
    t, y, has = series()
    with NativePf(model, n, SEED) as g:
        got = g.filter_intervals(t, y, has)
    o = oracle.OraclePf(model.descriptor(), n, SEED)
    o.init(float(np.min(t)))
    rows = [o.summary(0.975)]
    for s in range(len(t)):
        o.step(float(t[s]), float(y[s]), bool(has[s]))
        rows.append(o.summary(0.975))
    for j, name in enumerate(ROW_NAMES):
        want = np.array([r[j] for r in rows])
        if name in ("state_mean", "eta_of_mean"):                            # plain fp64 sums against the oracle's sequential sum: cssm_pf_summary's bound
            np.testing.assert_allclose(got[3 + j], want, rtol=1e-12, atol=1e-13, err_msg=name)
        else:
            np.testing.assert_array_equal(got[3 + j], want, err_msg=name)


# 3 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("interval", INTERVALS)
def test_clouds_that_break_a_selection(n, interval):
    """A d = 1 Brownian handle takes a crafted cloud (cssm_pf_adopt), then one record without a datum and dt = 0 through
    cssm_pf_filter_intervals_more.  The row, three ways: cssm_pf_summary on the same handle afterwards; exact order statistics from a
    sort of the order keys of get_particles(); the sequential twin.  (ranks: test_filter_intervals_host.ranks restates sel_ranks' rule.)"""
    assert ranks(n, 1.0, True) == (0, n - 1) and ranks(n, 1e-9, True) == (n - 1, 0) and ranks(n, 1e-9, False) == (n - 1, 0)
    by_name = {}
    with NativePf(cases.c1_model(), n, SEED) as g:
        g.init(0.0)
        for name, x in crafted_clouds(n, interval).items():
            g.adopt(x[None, :], 0.0, n)
            got = g.filter_intervals_more(np.array([0.0]), np.array([0.0]), np.array([0], dtype=np.uint8), interval)
            want = g.summary(interval)
            for j, rn in enumerate(ROW_NAMES):
                np.testing.assert_array_equal(got[3 + j][0], want[j], err_msg=f"{name}: {rn} against cssm_pf_summary")
            cloud = g.particles()[0]
            exact = exact_order_statistics(cloud, interval, True)
            twin, _ = twin_select(cloud, interval, True)
            lohi = np.array([got[4][0, 0], got[5][0, 0]])
            np.testing.assert_array_equal(lohi.view(np.uint64), exact.view(np.uint64), err_msg=f"{name}: against the sorted keys")
            np.testing.assert_array_equal(lohi.view(np.uint64), twin.view(np.uint64), err_msg=f"{name}: against the twin")
            by_name[name] = tuple(np.asarray(got[3 + j][0]).copy() for j in (1, 2, 4, 5))
    for other in ("multiset descending", "multiset shuffled"):              # one multiset, three orders: the same order statistics
        for a, b in zip(by_name["multiset ascending"], by_name[other]):
            np.testing.assert_array_equal(a, b, err_msg=other)


# 4 ------------------------------------------------------------------------------------------------------------------------------
def test_a_collapsed_cloud_from_the_filter_itself():
    """A Gaussian observation with a tiny scale leaves ESS = 1: the next row is N copies of one particle, reached through the ancestors."""
    model, n = cases.linear_model(obs_sd=1e-7), 4097
    t, y, has = np.array([0.0, 1.0, 2.0]), np.array([0.4, 0.45, 0.5]), np.ones(3, dtype=np.uint8)
    got = both_routes(model, n, t, y, has)
    assert got[2][0] == 1, got[2]
    assert got[4][1, 0] == got[5][1, 0] and got[7][1] == got[8][1]          # row 1: one value, lower == upper


# 5 ------------------------------------------------------------------------------------------------------------------------------
def test_a_held_and_redone_observation():
    """The outlying observation of tests/test_gpu_wave_sums.py: the series is put on hold at record 5, the host redoes it and enqueues the
    rest again -- the summary launches behind it returned at once, their rows are formed behind the redo."""
    t, y, has = cases.poisson_counts(9, missing=0.2)
    y = y.copy(); y[5] = 70.0; has = has.copy(); has[5] = 1
    both_routes(cases.c2_model(), 4096, t, y, has)
    with NativePf(cases.c2_model(), 4096, SEED) as a, NativePf(cases.c2_model(), 4096, SEED) as b:   # ... and inside a continued call
        a.init(0.0); b.init(0.0)
        got = a.filter_intervals_more(t, y, has)
        want = loop_rows(b, t, y, has, init=False)
        same_rows(got, want, "continued")
        same_handles(a, b, 10.0, "continued")


# 6 ------------------------------------------------------------------------------------------------------------------------------
def test_an_lgcp_handle():
    t, y, has = cases.event_times(6)
    both_routes(cases.c4_model(), 500, t, y, has, lgcp_precision=1)


@pytest.mark.parametrize("resampler", [1, 2])                                # stratified; multinomial (ancestors not sorted: the other gather pattern)
def test_stratified_and_multinomial_resamplers(resampler):
    t, y, has = series()
    both_routes(cases.c2_model(), 1000, t, y, has, option=(2, resampler))   # CSSM_OPT_RESAMPLER


# 7 ------------------------------------------------------------------------------------------------------------------------------
def test_step_intervals_stream_and_continued_calls():
    model, n = cases.c2_model(), 1000
    t, y, has = series()
    with NativePf(model, n, SEED) as g:
        whole = g.filter_intervals(t, y, has, 0.9)
        ms = g.intervals_last_ms()
        assert len(ms) == 2 and all(math.isfinite(v) and v > 0.0 for v in ms), ms
    with NativePf(model, n, SEED) as g:                                     # the stream: step_intervals per record
        g.init(float(np.min(t)))
        first = g.summary(0.9)
        rows = [g.step_intervals(float(t[s]), float(y[s]), bool(has[s]), 0.9) for s in range(len(t))]
        ms = g.intervals_last_ms()
        assert all(math.isfinite(v) and v > 0.0 for v in ms), ms
    np.testing.assert_array_equal(np.array([r[0] for r in rows]), whole[1])
    np.testing.assert_array_equal(np.array([r[1] for r in rows], dtype=np.int32), whole[2])
    for j, name in enumerate(ROW_NAMES):
        np.testing.assert_array_equal(np.array([first[j]] + [r[2 + j] for r in rows]), whole[3 + j], err_msg=name)
    with NativePf(model, n, SEED) as g:                                     # filter_intervals(t[:5]) then _more(t[5:]) = one call over all records
        a = g.filter_intervals(t[:5], y[:5], has[:5], 0.9)
        b = g.filter_intervals_more(t[5:], y[5:], has[5:], 0.9)
    assert b[0] == whole[0]
    for j in range(1, 9):
        np.testing.assert_array_equal(np.concatenate([a[j], b[j]]), whole[j], err_msg=str(j))


def test_filter_intervals_gives_the_pfouts_of_a_filter_stream():
    model, n = cases.c2_model(), 1000
    t, y, has = series()
    data = [Data(float(a), float(b) if h else None) for a, b, h in zip(t, y, has)]
    ll, outs = Filter(model, Resampling.systematicResampling, seed=SEED).filterIntervals(data, n)
    flt = Filter(model, Resampling.systematicResampling, seed=SEED)
    want, last = [], None
    for s in flt.filterStream(float(np.min(t)), n)(data):
        want.append(ParticleFilter.getIntervals(model, s)); last = s
    assert ll == last.ll and len(outs) == len(want) == len(data) + 1 and outs[0].observation is None
    for a, b in zip(outs, want):
        assert (a.time, a.observation, a.eta, a.etaIntervals, a.stateIntervals) == (b.time, b.observation, b.eta, b.etaIntervals, b.stateIntervals)
        np.testing.assert_array_equal(a.state, b.state)
    # stepIntervals: the stream with its PfOut per element
    f2 = Filter(model, Resampling.systematicResampling, seed=SEED)
    s = f2.initialiseState(n, float(np.min(t)))
    for k, dd in enumerate(data):
        s, out = f2.stepIntervals(s, dd)
        assert (out.time, out.eta, out.etaIntervals, out.stateIntervals) == (want[k + 1].time, want[k + 1].eta, want[k + 1].etaIntervals, want[k + 1].stateIntervals)
    assert s.ll == ll


# 8 ------------------------------------------------------------------------------------------------------------------------------
def test_refusals_by_code_and_message():
    lib = _abi.load_library()
    dp = C.POINTER(C.c_double)
    t, y, has = series()
    tp, yp = t.ctypes.data_as(dp), y.ctypes.data_as(dp)
    six = [None] * 6
    with NativePf(cases.c2_model(), 1000, SEED) as g:
        for fn in (lib.cssm_pf_filter_intervals, lib.cssm_pf_filter_intervals_more):
            assert fn(g._h, None, yp, None, 12, 0.975, None, None, None, *six) == _abi.CSSM_EINVAL_ARG and b"null argument" in lib.cssm_last_error()
            assert fn(g._h, tp, None, None, 12, 0.975, None, None, None, *six) == _abi.CSSM_EINVAL_ARG and b"null argument" in lib.cssm_last_error()
            assert fn(g._h, tp, yp, None, 0, 0.975, None, None, None, *six) == _abi.CSSM_EINVAL_ARG and b"empty data" in lib.cssm_last_error()
            for bad in (0.0, 1.5, float("nan")):
                assert fn(g._h, tp, yp, None, 12, bad, None, None, None, *six) == _abi.CSSM_EINVAL_ARG and b"interval must be in (0, 1]" in lib.cssm_last_error()
        assert lib.cssm_pf_filter_intervals_more(g._h, tp, yp, None, 12, 0.975, None, None, None, *six) == _abi.CSSM_ESTATE
        assert b"continuing a filter needs an initialised handle" in lib.cssm_last_error()
        assert lib.cssm_pf_step_intervals(g._h, 0.0, 1.0, 1, 0.975, None, None, *six) == _abi.CSSM_ESTATE and b"before cssm_pf_init" in lib.cssm_last_error()
        ms = np.full(2, 7.0)
        assert lib.cssm_pf_intervals_last_ms(g._h, ms.ctypes.data_as(dp)) == _abi.CSSM_ESTATE and list(ms) == [7.0, 7.0]
        with pytest.raises(CssmError):
            g.filter_intervals(t, y, has, interval=0.0)
        g.init(0.0)
        assert lib.cssm_pf_step_intervals(g._h, 1.0, 1.0, 1, 1.5, None, None, *six) == _abi.CSSM_EINVAL_ARG
        # every output may be null: the call still filters, and the handle is cssm_pf_ll_filter's
        ll = C.c_double()
        assert lib.cssm_pf_filter_intervals(g._h, tp, yp, has.ctypes.data_as(C.POINTER(C.c_uint8)), 12, 0.975, C.byref(ll), None, None, *six) == 0
        with NativePf(cases.c2_model(), 1000, SEED) as f:
            assert f.run(t, y, has)[0] == ll.value
            np.testing.assert_array_equal(f.particles(), g.particles())
    h = C.c_void_p()                                                         # the only shard of a cloud of 1000, on the default stream
    _abi.check(lib.cssm_pf_create_shard(cases.c2_model().descriptor().ptr(), 1000, 0, 1000, SEED, 0, None, C.byref(h)))
    try:
        assert lib.cssm_pf_filter_intervals(h, tp, yp, None, 12, 0.975, None, None, None, *six) == _abi.CSSM_ESTATE
        assert b"sharded handle" in lib.cssm_last_error()
    finally:
        lib.cssm_pf_destroy(h)
