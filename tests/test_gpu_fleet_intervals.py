"""-m gpu: filtered intervals of a whole fleet from the launch that filters it (include/cssm_pf.h: cssm_fleet_filter_intervals,
cssm_fleet_step_intervals; csrc/cssm_fleet_intervals.hip.h) -- examples/Filtering.scala:24-31 of every series: one PfOut per observation
and one for the initial cloud.

The expected values are the oracle's: OraclePf driven per series through init(t0), summary(interval), then step and summary for every
observation.  Order statistics, ll_t, ess_t and ll_out are compared with == / assert_array_equal.  Means are plain fp64 sums taken in
another order than the oracle's:
  * eta_of_mean under the exp and logistic links is held to the project's figure for such sums, rtol = 1e-12, atol = 0
    (tests/test_gpu_fleet.py, test_summaries);
  * a state component's mean can sit near zero (zero-mean seasonal and OU components), so it is bounded by what two summation orders of
    the same N numbers can differ by: each order errs by at most (N - 1) u sum|x_i| (u = 2^-53), each division by u |mean|, hence
    |delta mean| <= 2 N u mean(|x_i|), mean(|x_i|) taken from the oracle's cloud.  At N = 1 and N = 2 the bound is not needed (one
    rounding at most, the same in any order) and the comparison is ==.  Under the identity link (Model.linear of a one-dimensional
    state: f = 1) eta of the mean IS the state mean and takes its bound.
No series is skipped or excused; a status other than zero is asserted where the data provoke it and only there."""
import ctypes as C

import numpy as np
import pytest

import cases
from composablestatespacemodels_amd import Data, _abi
from composablestatespacemodels_amd.filter import FilterFleet, NativePfFleet, Resampling
from composablestatespacemodels_amd.formats import pfout_csv
from oracle import oracle
from test_gpu_fleet import assert_summary_equal_oracle
from test_gpu_fleet_interpolate import with_gap

pytestmark = pytest.mark.gpu

SEED = cases.SEED
U = 2.0 ** -53

_MODELS = {"c2": (cases.c2_model, cases.poisson_counts, "exp"), "linear": (cases.linear_model, cases.gaussian_series, "identity"),
           "bernoulli": (cases.bernoulli_model, cases.binary_series, "logistic"), "dim9": (lambda: cases.dim_model(9), cases.poisson_counts, "exp"),
           "dim16": (lambda: cases.dim_model(16), cases.poisson_counts, "exp")}


def ragged(gen):
    """five series: missing observations and a time step of its own; no records; repeated times (dt = 0); the smallest time is not the
    first record's (the time then runs backwards at record 2, which no model's transition survives: the series' own failure); one record"""
    out = []
    t, y, _ = gen(12, seed=SEED)
    has = np.array([1, 1, 0, 1, 0, 0, 1, 1, 0, 1, 1, 0], dtype=np.uint8)
    out.append((0.5 * t + 3.0, y, has))
    out.append((np.zeros(0), np.zeros(0), np.zeros(0, dtype=np.uint8)))
    t, y, _ = gen(7, seed=SEED + 2)
    out.append((np.array([0., 0., 1., 1., 1., 2.5, 2.5]), y, np.array([1, 1, 1, 0, 1, 1, 1], dtype=np.uint8)))
    t, y, _ = gen(4, seed=SEED + 3)
    out.append((np.array([2., 3., 1., 4.]), y, np.ones(4, dtype=np.uint8)))
    t, y, _ = gen(1, seed=SEED + 4)
    out.append((t + 7.25, y, np.ones(1, dtype=np.uint8)))
    return out


def oracle_rows(model, n, seed, data, intervals):
    """the oracle's PfOuts of one series: {interval: [summary of row 0, 1, ...]}, mean|x| per row, ll_t, ess_t, the index of the
    observation it could not weigh (or None), and the oracle itself"""
    t, y, has = data
    o = oracle.OraclePf(model.descriptor(), n, seed)
    rows, absx, ll_t, ess_t, failed = {iv: [] for iv in intervals}, [], [], [], None
    if len(t) == 0:
        return rows, absx, ll_t, ess_t, failed, o

    def record():
        for iv in intervals:
            rows[iv].append(o.summary(iv))
        absx.append(np.abs(o.particles()).mean(axis=1))
    o.init(float(np.min(t)))
    record()
    for s in range(len(t)):
        try:
            ll, ess = o.step(float(t[s]), float(y[s]), bool(has[s]))
        except oracle.OracleError:
            failed = s
            break
        ll_t.append(ll); ess_t.append(ess)
        record()
    return rows, absx, ll_t, ess_t, failed, o


def assert_rows(got, want, absx, n, link, tag):
    """one series' rows (mean, lower, upper, eta_of_mean, eta_lower, eta_upper) against the oracle's summaries, row by row"""
    m, lo, hi, em, el, eu = got
    for i, (om, olo, ohi, oem, oel, oeu) in enumerate(want):
        np.testing.assert_array_equal(lo[i], olo, err_msg=f"{tag} row {i} lower")
        np.testing.assert_array_equal(hi[i], ohi, err_msg=f"{tag} row {i} upper")
        assert (el[i], eu[i]) == (oel, oeu), (tag, i, el[i], eu[i], oel, oeu)
        bound = 2.0 * n * U * absx[i] if n > 2 else np.zeros_like(absx[i])
        delta = np.abs(m[i] - om)
        assert np.all(delta <= bound), (tag, i, m[i], om, delta, bound)
        if link == "identity":
            assert abs(em[i] - oem) <= bound[0], (tag, i, em[i], oem, bound[0])
        else:
            np.testing.assert_allclose(em[i], oem, rtol=1e-12, atol=0, err_msg=f"{tag} row {i} eta of the mean")


def assert_nan_rows(got, first, tag):
    for a in got:
        assert np.isnan(a[first:]).all(), (tag, first, a)


# 1 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 63, 100, 1000, _abi.FLEET_MAX_N])
@pytest.mark.parametrize("name", list(_MODELS))
def test_every_row_of_a_ragged_fleet_equals_the_oracle(name, n):
    make, gen, link = _MODELS[name]
    model = make()
    datas = ragged(gen)
    S = len(datas)
    seeds = [SEED + 17 * k for k in range(S)]
    intervals = (0.975, 0.5, 1.0)
    want = [oracle_rows(model, n, seeds[k], datas[k], intervals) for k in range(S)]
    assert want[3][4] == 2, "the premise: the oracle cannot move series 3 backwards in time either"
    assert [w[4] for k, w in enumerate(want) if k != 3] == [None] * (S - 1)
    with NativePfFleet(model, n, S) as fl:
        fl.reseed(seeds)
        for iv in intervals:
            ll, ll_t, ess_t, rows, rc = fl.filter_intervals(datas, iv)
            assert list(rc) == [0, _abi.CSSM_EINVAL_ARG, 0, _abi.CSSM_ENONFINITE, 0], rc
            for k in range(S):
                wrows, absx, oll_t, oess_t, failed, o = want[k]
                T = len(datas[k][0])
                assert all(len(a) == T + 1 for a in rows[k])
                if T == 0:
                    assert np.isnan(ll[k])
                    assert_nan_rows(rows[k], 0, (name, n, iv, k))
                    continue
                seen = T if failed is None else failed
                np.testing.assert_array_equal(ll_t[k][:seen], oll_t)
                np.testing.assert_array_equal(ess_t[k][:seen], oess_t)
                assert_rows(rows[k], wrows[iv], absx, n, link, (name, n, iv, k))
                assert len(wrows[iv]) == seen + 1
                if failed is None:
                    assert ll[k] == oll_t[-1]
                    np.testing.assert_array_equal(fl.particles(k), o.particles())
                    np.testing.assert_array_equal(fl.ancestors(k), o.ancestors())
                else:
                    assert np.isnan(ll[k]) and np.isnan(ll_t[k][seen:]).all() and (ess_t[k][seen:] == -1).all()
                    assert_nan_rows(rows[k], seen + 1, (name, n, iv, k))


def assert_whole_series_equals_the_oracle(fl, k, res, want, iv, n, link, tag):
    """series k of a `filter_intervals(datas, iv)` that the oracle ran to its end (want: its oracle_rows): every row, ll_t, ess_t, ll and
    the cloud the fleet holds afterwards"""
    ll, ll_t, ess_t, rows, rc = res
    wrows, absx, oll_t, oess_t, failed, o = want
    assert rc[k] == 0 and failed is None, (tag, rc[k], failed)
    assert all(len(a) == len(oll_t) + 1 for a in rows[k]) and len(wrows[iv]) == len(oll_t) + 1
    np.testing.assert_array_equal(ll_t[k], oll_t)
    np.testing.assert_array_equal(ess_t[k], oess_t)
    assert_rows(rows[k], wrows[iv], absx, n, link, tag)
    assert ll[k] == oll_t[-1]
    np.testing.assert_array_equal(fl.particles(k), o.particles())
    np.testing.assert_array_equal(fl.ancestors(k), o.ancestors())


@pytest.mark.parametrize("d", list(range(1, 17)))
def test_every_latent_dimension(d):
    """k_fleet_series<d, IVAL> from both entry points and k_fleet_summary<d>: the per-dimension fixture of the sibling files (two
    unweighted records: the None branch has an IVAL call site of its own), every row against the oracle; then two streamed records in
    which the three series are weighted, unweighted and inactive in turn, against the oracle's step + summary and, bit for bit, a twin
    fleet's step + summary -- whose summaries are held to the oracle by test_summaries' rules as well."""
    model = cases.dim_model(d)
    S, n = 3, 257
    seeds = [SEED + 17 * k for k in range(S)]
    datas = [with_gap(cases.poisson_counts(6, seed=SEED + k), 2, 4) for k in range(S)]
    intervals = (0.975, 0.5, 1.0)
    want = [oracle_rows(model, n, seeds[k], datas[k], intervals) for k in range(S)]
    orc = [w[5] for w in want]
    with NativePfFleet(model, n, S) as fl, NativePfFleet(model, n, S) as tw:
        assert fl.d == tw.d == d
        fl.reseed(seeds); tw.reseed(seeds)
        for iv in intervals:
            res = fl.filter_intervals(datas, iv)
            assert not res[4].any(), res[4]
            for k in range(S):
                assert_whole_series_equals_the_oracle(fl, k, res, want[k], iv, n, "exp", (d, iv, k))
        _, _, _, rc = tw.ll_filter(datas)
        assert not rc.any(), rc
        sm = tw.summary(1.0)
        for k in range(S):
            assert_summary_equal_oracle(sm, k, orc[k], 1.0)
            for a, b in zip(res[3][k], sm):                      # the call's last row is the summary of the cloud it leaves
                np.testing.assert_array_equal(a[-1], b[k])
        clock = np.array([float(dd[0][-1]) for dd in datas])
        for r, interval in enumerate((0.975, 0.5)):
            role = [(k + r) % 3 for k in range(S)]               # 0: weighted, 1: unweighted, 2: inactive
            active = np.array([q != 2 for q in role], dtype=np.uint8)
            has = np.array([q == 0 for q in role], dtype=np.uint8)
            clock = clock + np.where(active != 0, 0.5 + 0.25 * r, 0.0)
            y = np.array([2.0, 0.0, 4.0])
            ll, ess, rows, rc = _raw_step_intervals(fl, clock, y, has, active, interval, 7.5)
            lb, eb, rb = tw.step(clock, y, has, active)
            sb = tw.summary(interval)
            assert not rc.any() and not rb.any(), (r, rc, rb)
            for k in range(S):
                if not active[k]:                                # untouched: the sentinels stand
                    assert ll[k] == 7.5 and ess[k] == -77 and all(np.all(a[k] == 7.5) for a in rows), (r, k)
                    continue
                assert (ll[k], ess[k]) == (lb[k], eb[k]) == orc[k].step(clock[k], y[k], bool(has[k])), (d, r, k)
                for a, b in zip(rows, sb):
                    np.testing.assert_array_equal(a[k], b[k], err_msg=f"d {d} round {r} series {k}")
                got = tuple(np.asarray(a[k])[None] for a in rows)
                assert_rows(got, [orc[k].summary(interval)], [np.abs(orc[k].particles()).mean(axis=1)], n, "exp", (d, r, k))
                assert_summary_equal_oracle(sb, k, orc[k], interval)
        for k in range(S):
            for f in (fl, tw):
                np.testing.assert_array_equal(f.particles(k), orc[k].particles())
                np.testing.assert_array_equal(f.ancestors(k), orc[k].ancestors())
            assert fl.observation_index(k) == tw.observation_index(k)


# 2 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [100, 1000])
def test_a_series_that_fails_mid_way_keeps_its_rows_and_nobody_notices(n):
    """series 2's observation 3 is an outlier no particle can be weighed against (as tests/test_gpu_fleet.py provokes the status): rows
    0 .. 3 are the oracle's, rows 4 .. are NaN, and the neighbours are bit for bit the same fleet without it"""
    model = cases.linear_model()
    S = 4
    seeds = [SEED + 17 * k for k in range(S)]
    datas = [cases.gaussian_series(6 + k, seed=SEED + k) for k in range(S)]
    bad = datas[2][1].copy(); bad[3] = 1e200
    datas[2] = (datas[2][0], bad, datas[2][2])
    keep = [0, 1, 3]
    with NativePfFleet(model, n, S) as fl, NativePfFleet(model, n, 3) as f3:
        fl.reseed(seeds); f3.reseed([seeds[k] for k in keep])
        ll, ll_t, ess_t, rows, rc = fl.filter_intervals(datas, 0.9)
        ll3, ll_t3, ess_t3, rows3, rc3 = f3.filter_intervals([datas[k] for k in keep], 0.9)
        assert list(rc) == [0, 0, _abi.CSSM_ENONFINITE, 0] and not rc3.any()
        for j, k in enumerate(keep):
            assert ll[k] == ll3[j]
            np.testing.assert_array_equal(ll_t[k], ll_t3[j]); np.testing.assert_array_equal(ess_t[k], ess_t3[j])
            for a, b in zip(rows[k], rows3[j]):
                np.testing.assert_array_equal(a, b)
            np.testing.assert_array_equal(fl.particles(k), f3.particles(j))
            wrows, absx, oll_t, oess_t, failed, o = oracle_rows(model, n, seeds[k], datas[k], (0.9,))
            assert failed is None and ll[k] == oll_t[-1]
            assert_rows(rows[k], wrows[0.9], absx, n, "identity", (n, k))
        wrows, absx, oll_t, oess_t, failed, _ = oracle_rows(model, n, seeds[2], datas[2], (0.9,))
        assert failed == 3                                       # (the premise: the oracle cannot weigh that observation either)
        assert len(wrows[0.9]) == 4
        assert_rows(rows[2], wrows[0.9], absx, n, "identity", (n, 2))
        assert_nan_rows(rows[2], 4, (n, 2))
        np.testing.assert_array_equal(ll_t[2][:3], oll_t)
        assert np.isnan(ll[2]) and np.isnan(ll_t[2][3:]).all()


# 3 ------------------------------------------------------------------------------------------------------------------------------
def _good(datas):
    return [d for k, d in enumerate(datas) if k in (0, 2, 4)]


@pytest.mark.parametrize("n", [100, 1000])
def test_the_fleet_afterwards_is_the_one_ll_filter_leaves(n):
    model = cases.c2_model()
    datas = _good(ragged(cases.poisson_counts))
    S = len(datas)
    seeds = [SEED + 17 * k for k in range(S)]
    with NativePfFleet(model, n, S) as fa, NativePfFleet(model, n, S) as fb:
        fa.reseed(seeds); fb.reseed(seeds)
        ll, ll_t, ess_t, rows, rc = fa.filter_intervals(datas, 0.8)
        llb, ll_tb, ess_tb, rcb = fb.ll_filter(datas)
        assert not rc.any() and not rcb.any()
        np.testing.assert_array_equal(ll, llb)
        sb = fb.summary(0.8)
        for k in range(S):
            np.testing.assert_array_equal(ll_t[k], ll_tb[k]); np.testing.assert_array_equal(ess_t[k], ess_tb[k])
            np.testing.assert_array_equal(fa.particles(k), fb.particles(k))
            np.testing.assert_array_equal(fa.ancestors(k), fb.ancestors(k))
            assert fa.observation_index(k) == fb.observation_index(k) == len(datas[k][0])
            # the call's last row is cssm_fleet_summary of the cloud it leaves: order statistics bit for bit -- and the means too, because
            # the block adds a row's values in k_fleet_summary's order (csrc/cssm_fleet_intervals.hip.h)
            for a, b in zip(rows[k], sb):
                np.testing.assert_array_equal(a[-1], b[k])
        sa = fa.summary(0.8)
        for a, b in zip(sa, sb):
            np.testing.assert_array_equal(a, b)
        t = np.array([d[0][-1] + 0.75 for d in datas]); y = np.array([1.0, 3.0, 0.0])
        la, ea, ra = fa.step(t, y)
        lb, eb, rb = fb.step(t, y)
        assert not ra.any() and not rb.any()
        np.testing.assert_array_equal(la, lb); np.testing.assert_array_equal(ea, eb)
        for a, b in zip(fa.summary(0.975), fb.summary(0.975)):
            np.testing.assert_array_equal(a, b)
        for k in range(S):
            np.testing.assert_array_equal(fa.particles(k), fb.particles(k))
        assert fa.last_ms()[0] > 0.0 and len(fa.last_ms()) == 3


# 4 ------------------------------------------------------------------------------------------------------------------------------
def _raw_step_intervals(fl, t, y, has, active, interval, sentinel):
    """cssm_fleet_step_intervals through the C ABI with every output preset to a sentinel of the test's own"""
    S, d = fl.S, fl.d
    p = lambda a, ty=C.c_double: a.ctypes.data_as(C.POINTER(ty))
    ll = np.full(S, sentinel); ess = np.full(S, -77, dtype=np.int32); rc = np.full(S, -77, dtype=np.int32)
    m, lo, hi = (np.full((S, d), sentinel) for _ in range(3))
    em, el, eu = (np.full(S, sentinel) for _ in range(3))
    assert fl.lib.cssm_fleet_step_intervals(fl._h, p(active, C.c_uint8), p(t), p(y), p(has, C.c_uint8), interval, p(ll), p(ess, C.c_int32),
                                            p(m), p(lo), p(hi), p(em), p(el), p(eu), p(rc, C.c_int)) == 0, fl.lib.cssm_last_error()
    return ll, ess, (m, lo, hi, em, el, eu), rc


@pytest.mark.parametrize("name,n", [("c2", 100), ("c2", 1000), ("dim9", 100), ("linear", _abi.FLEET_MAX_N), ("bernoulli", 2)])
def test_streaming_steps_with_intervals_equal_step_then_summary(name, n):
    make, gen, link = _MODELS[name]
    model = make()
    S, rounds = 5, 8
    seeds = [SEED + 17 * k for k in range(S)]
    ys = [gen(rounds, seed=SEED + k)[1] for k in range(S)]
    clock = np.array([0.5 * k for k in range(S)])
    orc = [oracle.OraclePf(model.descriptor(), n, seeds[k]) for k in range(S)]
    with NativePfFleet(model, n, S) as fa, NativePfFleet(model, n, S) as fb:
        fa.reseed(seeds); fb.reseed(seeds)
        fa.init(clock); fb.init(clock)
        for k in range(S):
            orc[k].init(clock[k])
        for r in range(rounds):
            interval = (0.975, 0.6, 1.0)[r % 3]
            active = np.array([(r + k) % 3 != 0 for k in range(S)], dtype=np.uint8)
            has = np.array([(r * 5 + k) % 4 != 0 for k in range(S)], dtype=np.uint8)
            clock = clock + np.where(active != 0, 0.25 * ((r + np.arange(S)) % 3), 0.0)      # (dt = 0 among them)
            y = np.array([ys[k][r] for k in range(S)])
            ll, ess, rows, rc = _raw_step_intervals(fa, clock, y, has, active, interval, 7.5)
            lb, eb, rb = fb.step(clock, y, has, active)
            sb = fb.summary(interval)
            assert not rc.any() and not rb.any(), (r, rc, rb)
            for k in range(S):
                if not active[k]:                                # untouched: the sentinels stand
                    assert ll[k] == 7.5 and ess[k] == -77 and all(np.all(a[k] == 7.5) for a in rows), (r, k)
                    continue
                assert ll[k] == lb[k] and ess[k] == eb[k], (r, k)
                for a, b in zip(rows, sb):                       # order statistics bit for bit; the means too (k_fleet_summary's order)
                    np.testing.assert_array_equal(a[k], b[k], err_msg=f"round {r} series {k}")
                ol, oess = orc[k].step(clock[k], y[k], bool(has[k]))
                assert (ll[k], ess[k]) == (ol, oess), (r, k)
                got = tuple(np.asarray(a[k])[None] for a in rows)
                assert_rows(got, [orc[k].summary(interval)], [np.abs(orc[k].particles()).mean(axis=1)], n, link, (name, n, r, k))
        for k in range(S):
            np.testing.assert_array_equal(fa.particles(k), fb.particles(k))
            np.testing.assert_array_equal(fa.ancestors(k), fb.ancestors(k))
            assert fa.observation_index(k) == fb.observation_index(k)


# 5 ------------------------------------------------------------------------------------------------------------------------------
def test_filter_fleet_writes_the_references_filtered_csv_lines():
    """FilterFleet.filterIntervals: T_k + 1 PfOuts per series, the first without an observation at t0; their pfout_csv lines are those of
    initialiseState / stepFilter + getIntervals in a loop, and stepIntervals gives the same PfOuts a step at a time"""
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
        outs = ff.filterIntervals(datas)
    assert [len(o) for o in outs] == [len(d) + 1 for d in datas]
    for k in range(S):
        assert outs[k][0].observation is None and outs[k][0].time == t0[k]
        assert [o.observation for o in outs[k][1:]] == [d.observation for d in datas[k]]
        assert [o.time for o in outs[k][1:]] == [d.t for d in datas[k]]
    lines = [[pfout_csv(o) for o in outs[k]] for k in range(S)]
    with FilterFleet(mods, Resampling.systematicResampling, n, seed=SEED) as ff, FilterFleet(mods, Resampling.systematicResampling, n, seed=SEED) as fs:
        st = ff.initialiseState(t0); ss = fs.initialiseState(t0)
        loop = [[pfout_csv(o)] for o in ff.getIntervals()]
        stream = [[line[0]] for line in loop]
        for r in range(max(len(d) for d in datas)):
            obs = [d[r] if r < len(d) else None for d in datas]
            st = ff.stepFilter(st, obs)
            got = ff.getIntervals()
            ss, souts = fs.stepIntervals(ss, obs)
            for k in range(S):
                if obs[k] is not None:
                    loop[k].append(pfout_csv(got[k]))
                    stream[k].append(pfout_csv(souts[k]))
                else:
                    assert souts[k] is None
    assert lines == loop
    assert lines == stream
