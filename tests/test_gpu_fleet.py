"""-m gpu: the fleet filter (include/cssm_pf.h: cssm_fleet_*, csrc/cssm_fleet.hip): S small series per launch, one workgroup each --
the reference's everyday shape (a streaming filter per sensor, examples/Filtering.scala:24; the pilot run of model/Streaming.scala:19-40).
Per series the results must be those of the oracle and of a handle of its own, bit for bit: every comparison below is == /
assert_array_equal unless it says otherwise, no series is skipped or excused, and every rc is zero where the test does not provoke one."""
import ctypes as C

import numpy as np
import pytest

import cases
from composablestatespacemodels_amd import CssmError, Data, Streaming, _abi
from composablestatespacemodels_amd.filter import FilterFleet, NativePf, NativePfFleet, Resampling
from oracle import oracle

pytestmark = pytest.mark.gpu

SEED = cases.SEED


def run_key(seed, k):
    return int(oracle.lib().oracle_c_derive_key(seed, k))


def _perturbed(make_params, k):
    """series k's parameters: the model's own, shifted a little per series (the structures stay equal)"""
    p = make_params()
    th = np.asarray(p.flattenParams())
    return p.withFlat(th + 0.03 * (k % 7) * np.cos(np.arange(th.size) + k))


def ragged_c2(S=24):
    """test 1's fleet: models, seeds and ragged data (different lengths, time steps, origins and missing patterns)"""
    um = cases.c2_unparam()
    models = [um.run(_perturbed(cases.c2_params, k)) for k in range(S)]
    seeds = [SEED + 17 * k for k in range(S)]
    datas = []
    for k in range(S):
        t, y, has = cases.poisson_counts(5 + (7 * k) % 23, seed=SEED + k, dt=(1, .5, .25)[k % 3], missing=(0, .15, .4)[k % 3])
        datas.append((t + 3.0 * (k % 4), y, has))
    return models, seeds, datas


def assert_series_equal_oracle(fl, k, model, n, seed, data, ll, ll_t, ess_t, native=False):
    o = oracle.OraclePf(model.descriptor(), n, seed)
    ol, oll_t, oess_t, _ = o.filter(*data)
    assert ll[k] == ol, (k, n, ll[k], ol)
    np.testing.assert_array_equal(ll_t[k], oll_t)
    np.testing.assert_array_equal(ess_t[k], oess_t)
    np.testing.assert_array_equal(fl.particles(k), o.particles())
    np.testing.assert_array_equal(fl.ancestors(k), o.ancestors())
    if native:
        with NativePf(model, n, seed) as g:
            gl, gll_t, gess_t, _ = g.run(*data)
            assert ll[k] == gl
            np.testing.assert_array_equal(ll_t[k], gll_t)
            np.testing.assert_array_equal(ess_t[k], gess_t)
            np.testing.assert_array_equal(fl.particles(k), g.particles())
            np.testing.assert_array_equal(fl.ancestors(k), g.ancestors())
    return o


def assert_summary_equal_oracle(got, k, o, interval):
    """series k of a `summary(interval)` (six arrays over the series) against the oracle's summary of the same cloud: test_summaries'
    rules -- order statistics bit for bit, the means (plain fp64 sums in another order) within rtol 1e-12, atol 0"""
    m, lo, hi, em, el, eu = got
    om, olo, ohi, oem, oel, oeu = o.summary(interval)
    np.testing.assert_array_equal(lo[k], olo)
    np.testing.assert_array_equal(hi[k], ohi)
    assert el[k] == oel and eu[k] == oeu
    np.testing.assert_allclose(m[k], om, rtol=1e-12, atol=0)      # plain fp64 sums in another order
    np.testing.assert_allclose(em[k], oem, rtol=1e-12, atol=0)


# 1 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 63, 100, 1000, _abi.FLEET_MAX_N])
def test_ragged_fleet_equals_the_oracle_and_handles_of_its_own(n):
    S = 24
    models, seeds, datas = ragged_c2(S)
    with NativePfFleet(models[0], n, S) as fl:
        fl.set_params(models)
        for sd in (seeds, seeds[1:] + seeds[:1]):            # the same fleet again with the seeds rotated by one (buffers reused)
            fl.reseed(sd)
            ll, ll_t, ess_t, rc = fl.ll_filter(datas)
            assert not rc.any(), rc
            for k in range(S):
                assert_series_equal_oracle(fl, k, models[k], n, sd[k], datas[k], ll, ll_t, ess_t, native=n in (100, _abi.FLEET_MAX_N))


# 2 ------------------------------------------------------------------------------------------------------------------------------
_GEN = {"c1": cases.poisson_counts, "c2": cases.poisson_counts, "c3": cases.poisson_counts, "negbin": cases.poisson_counts,
        "euler": cases.poisson_counts, "linear": cases.gaussian_series, "studentt": cases.gaussian_series, "gbsg": cases.gaussian_series,
        "zip": cases.counts_with_zeros, "bernoulli": cases.binary_series, "beta": cases.unit_interval_series}


@pytest.mark.parametrize("name", [n for n in cases.GOLDEN_NAMES if n != "c4"] + ["gbsg", "euler"])
def test_every_served_observation_model(name):
    model = cases.literal_case(name, 12)[0]
    S, n, T = 5, 1000, 12
    seeds = [SEED + 17 * k for k in range(S)]
    datas = [_GEN[name](T, seed=SEED + k) for k in range(S)]
    with NativePfFleet(model, n, S) as fl:
        fl.reseed(seeds)
        ll, ll_t, ess_t, rc = fl.ll_filter(datas)
        assert not rc.any(), rc
        for k in range(S):
            assert_series_equal_oracle(fl, k, model, n, seeds[k], datas[k], ll, ll_t, ess_t)


@pytest.mark.parametrize("d", list(range(1, 17)))
def test_every_latent_dimension(d):
    model = cases.dim_model(d)
    S, n = 3, 257
    seeds = [SEED + 17 * k for k in range(S)]
    datas = [cases.poisson_counts(6, seed=SEED + k) for k in range(S)]
    with NativePfFleet(model, n, S) as fl:
        assert fl.d == d
        fl.reseed(seeds)
        ll, ll_t, ess_t, rc = fl.ll_filter(datas)
        assert not rc.any(), rc
        for k in range(S):
            assert_series_equal_oracle(fl, k, model, n, seeds[k], datas[k], ll, ll_t, ess_t)


# 3 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [100, 1000, _abi.FLEET_MAX_N])
def test_the_level_is_chosen_in_the_block(n):
    """Series 1's observation 4 is an outlier (c - max beyond CSSM_REF_ABOVE): its level is the max, found in place -- the single
    handle redoes such an observation, the batch holds the chain."""
    model = cases.c2_model()
    S = 3
    seeds = [SEED + 17 * k for k in range(S)]
    t, y, has = cases.poisson_counts(10)
    y1 = y.copy(); y1[4] = 60.0
    datas = [(t, y, has), (t, y1, has), (t, y, has)]
    o = oracle.OraclePf(model.descriptor(), n, seeds[1])     # (the premise, on the oracle: the level of that observation IS the max)
    o.init(t[0])
    for s in range(5):
        o.step(t[s], y1[s], bool(has[s]))
    ref, gmax = o.ref()
    assert ref == gmax and o.ref_level(60.0) - gmax > 32.0
    with NativePfFleet(model, n, S) as fl:
        fl.reseed(seeds)
        ll, ll_t, ess_t, rc = fl.ll_filter(datas)
        assert not rc.any(), rc
        for k in range(S):
            assert_series_equal_oracle(fl, k, model, n, seeds[k], datas[k], ll, ll_t, ess_t)


# 4 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["c2", "linear"])
def test_streaming_steps_with_clocks_and_patterns_of_their_own(which):
    model, gen = (cases.c2_model(), cases.poisson_counts) if which == "c2" else (cases.linear_model(), cases.gaussian_series)
    S, n, rounds = 16, 1000, 30
    keys = [run_key(SEED, k) for k in range(S)]
    ys = [gen(rounds, seed=SEED + k)[1] for k in range(S)]
    orc = [oracle.OraclePf(model.descriptor(), n, keys[k]) for k in range(S)]
    clock = np.array([0.5 * k for k in range(S)])
    with NativePfFleet(model, n, S) as fl:
        fl.reseed(keys)
        fl.init(clock)
        for k in range(S):
            orc[k].init(clock[k])
        for r in range(rounds):
            active = np.array([(r + k) % 3 != 0 for k in range(S)], dtype=np.uint8)
            has = np.array([(r * 5 + k) % 4 != 0 for k in range(S)], dtype=np.uint8)
            for k in range(S):
                if active[k]:
                    clock[k] += 0.25 * (1 + (r + k) % 4)
            y = np.array([ys[k][r] for k in range(S)])
            ll, ess, rc = fl.step(clock, y, has, active)
            assert not rc.any(), (r, rc)
            for k in range(S):
                if active[k]:
                    ol, oess = orc[k].step(clock[k], y[k], bool(has[k]))
                    assert ll[k] == ol, (r, k, ll[k], ol)
                    assert ess[k] == oess, (r, k)
        for k in range(S):
            np.testing.assert_array_equal(fl.particles(k), orc[k].particles())
            np.testing.assert_array_equal(fl.ancestors(k), orc[k].ancestors())


def test_ll_filter_continues_with_step():
    """ll_filter of the first half of every series followed by step through the second half equals ll_filter of the whole (the rule
    cssm_pf_ll_filter_more states for handles)."""
    S, n = 24, 1000
    models, seeds, datas = ragged_c2(S)
    half = [len(d[0]) // 2 for d in datas]
    with NativePfFleet(models[0], n, S) as fl:
        fl.set_params(models); fl.reseed(seeds)
        ll, _, _, rc = fl.ll_filter([tuple(a[:half[k]] for a in datas[k]) for k in range(S)])
        assert not rc.any()
        for r in range(max(len(d[0]) - h for d, h in zip(datas, half))):
            idx = [half[k] + r for k in range(S)]
            active = np.array([idx[k] < len(datas[k][0]) for k in range(S)], dtype=np.uint8)
            pick = lambda j: np.array([datas[k][j][idx[k]] if active[k] else 0 for k in range(S)])
            l2, _, rc = fl.step(pick(0).astype(np.float64), pick(1).astype(np.float64), pick(2).astype(np.uint8), active)
            assert not rc.any()
            ll = np.where(active != 0, l2, ll)
        for k in range(S):
            o = oracle.OraclePf(models[k].descriptor(), n, seeds[k])
            ol = o.filter(*datas[k])[0]
            assert ll[k] == ol, (k, ll[k], ol)
            np.testing.assert_array_equal(fl.particles(k), o.particles())
            np.testing.assert_array_equal(fl.ancestors(k), o.ancestors())


# 5 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [100, 1000])
def test_one_series_fails_and_the_others_do_not_notice(n):
    model = cases.linear_model()
    S = 4
    seeds = [SEED + 17 * k for k in range(S)]
    datas = [cases.gaussian_series(8, seed=SEED + k) for k in range(S)]
    bad = datas[2][1].copy(); bad[3] = 1e200
    datas[2] = (datas[2][0], bad, datas[2][2])
    with NativePfFleet(model, n, S) as fl:
        fl.reseed(seeds)
        ll, ll_t, ess_t, rc = fl.ll_filter(datas)
        assert list(rc) == [0, 0, _abi.CSSM_ENONFINITE, 0]
        for k in (0, 1, 3):
            assert_series_equal_oracle(fl, k, model, n, seeds[k], datas[k], ll, ll_t, ess_t)
        o = oracle.OraclePf(model.descriptor(), n, seeds[2])
        with pytest.raises(oracle.OracleError):
            o.filter(*datas[2])                              # (the premise: the oracle cannot weigh that observation either)
        o.init(datas[2][0][0])
        for s in range(3):
            ol, oess = o.step(datas[2][0][s], datas[2][1][s], True)
            assert ll_t[2][s] == ol and ess_t[2][s] == oess
        with pytest.raises(CssmError):
            fl.particles(2)                                  # its cloud is undefined until it is initialised again
        # after init the fleet runs again correctly, series 2 included
        fl.init(np.zeros(S))
        datas2 = [cases.gaussian_series(5 + 3 * k, seed=SEED + 100 + k, dt=(1, .5)[k % 2]) for k in range(S)]
        ll, ll_t, ess_t, rc = fl.ll_filter(datas2)
        assert not rc.any()
        for k in range(S):
            assert_series_equal_oracle(fl, k, model, n, seeds[k], datas2[k], ll, ll_t, ess_t)


# 6 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 1000, _abi.FLEET_MAX_N])
def test_summaries(n):
    S = 24
    models, seeds, datas = ragged_c2(S)
    with NativePfFleet(models[0], n, S) as fl:
        fl.set_params(models); fl.reseed(seeds)
        _, _, _, rc = fl.ll_filter(datas)
        assert not rc.any()
        orc = []
        for k in range(S):
            o = oracle.OraclePf(models[k].descriptor(), n, seeds[k]); o.filter(*datas[k]); orc.append(o)
        for interval in (0.975, 0.5):
            got = fl.summary(interval)
            for k in range(S):
                assert_summary_equal_oracle(got, k, orc[k], interval)


# 7 ------------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_reason_and_leave_the_fleet_usable():
    model = cases.c2_model()

    def refused(code, word, fn):
        with pytest.raises(CssmError) as e:
            fn()
        assert e.value.code == code and word in str(e.value), str(e.value)

    refused(_abi.CSSM_EINVAL_DESC, "LGCP", lambda: NativePfFleet(cases.c4_model(), 100, 2))
    refused(_abi.CSSM_EINVAL_ARG, "particles", lambda: NativePfFleet(model, 0, 2))
    refused(_abi.CSSM_EINVAL_ARG, "cssm_pf_", lambda: NativePfFleet(model, _abi.FLEET_MAX_N + 1, 2))
    refused(_abi.CSSM_EINVAL_ARG, "series", lambda: NativePfFleet(model, 100, 0))
    for rs in (Resampling.stratifiedResampling, Resampling.multinomialResampling, Resampling.residualResampling, lambda p, w: p):
        refused(_abi.CSSM_EINVAL_ARG, "systematic", lambda: FilterFleet([model, model], rs, 100))
    S, n = 3, 100
    seeds = [SEED + 17 * k for k in range(S)]
    datas = [cases.poisson_counts(6, seed=SEED + k) for k in range(S)]
    with NativePfFleet(model, n, S) as fl:
        fl.reseed(seeds)
        t = np.zeros(S); rc = np.zeros(S, dtype=np.int32)
        refused(_abi.CSSM_ESTATE, "initialised", lambda: fl.step(t, t))                       # step before init
        refused(_abi.CSSM_EINVAL_DESC, "structure", lambda: fl.set_params([model, cases.c1_model(), model]))
        off = np.array([0, 6, 4, 10], dtype=np.uint64); tt = np.zeros(10); ll = np.zeros(S)
        p = lambda a, ty: a.ctypes.data_as(C.POINTER(ty))
        assert fl.lib.cssm_fleet_ll_filter(fl._h, p(off, C.c_uint64), p(tt, C.c_double), p(tt, C.c_double), None, p(ll, C.c_double), None, None,
                                           p(rc, C.c_int)) == _abi.CSSM_EINVAL_ARG
        assert b"non-decreasing" in fl.lib.cssm_last_error()
        refused(_abi.CSSM_EINVAL_ARG, "systematic", lambda: fl.set_option(2, 1))
        ll, ll_t, ess_t, rc = fl.ll_filter(datas)            # still usable, with the parameters it had
        assert not rc.any()
        for k in range(S):
            assert_series_equal_oracle(fl, k, model, n, seeds[k], datas[k], ll, ll_t, ess_t)


# 8 ------------------------------------------------------------------------------------------------------------------------------
def test_pilot_run_variances():
    model = cases.c2_model()
    t, y, has = cases.poisson_counts(30, missing=0.1)
    data = [Data(float(a), float(b) if h else None) for a, b, h in zip(t, y, has)]
    particles, R = (100, 400, 1600, 8192), 16
    got = Streaming.pilotRun(data, model, particles, R, SEED)
    assert [n for n, _ in got] == list(particles)
    for n, v in got:
        lls = []
        for r in range(R):
            with NativePf(model, n, run_key(SEED, r)) as g:
                lls.append(g.run(t, y, has)[0])
        assert v == float(np.var(np.asarray(lls), ddof=1)), (n, v)
    assert got[0][1] > got[1][1] > got[2][1] > 0.0           # (a key reused across repetitions would flatten this)


# 9 ------------------------------------------------------------------------------------------------------------------------------
def test_scale_more_blocks_than_the_gpu_holds():
    model = cases.c1_model()
    S, n, T = 4096, 1000, 50
    keys = [run_key(SEED, k) for k in range(S)]
    datas = [cases.poisson_counts(T, seed=SEED + k) for k in range(S)]
    with NativePfFleet(model, n, S) as fl:
        fl.reseed(keys)
        ll, ll_t, ess_t, rc = fl.ll_filter(datas)
        assert not rc.any()
        for k in range(0, S, 128):
            assert_series_equal_oracle(fl, k, model, n, keys[k], datas[k], ll, ll_t, ess_t)


def test_filter_fleet_in_the_reference_vocabulary():
    """FilterFleet: initialiseState / stepFilter with a sensor that has nothing new / llFilter / getIntervals, series k under
    cssm_pf_run_key(seed, k), against one Filter-like oracle per sensor."""
    um = cases.c2_unparam()
    S, n = 4, 500
    mods = [um.run(_perturbed(cases.c2_params, k)) for k in range(S)]
    with FilterFleet(mods, Resampling.systematicResampling, n, seed=SEED) as ff:
        orc = [oracle.OraclePf(mods[k].descriptor(), n, run_key(SEED, k)) for k in range(S)]
        st = ff.initialiseState([0.0, 1.0, 2.0, 3.0])
        for k in range(S):
            orc[k].init(float(k))
        for r in range(6):
            obs = [None if (r + k) % 3 == 0 else Data(k + 0.5 * (r + 1), None if (r + k) % 4 == 1 else float((r * 3 + k) % 5)) for k in range(S)]
            st = ff.stepFilter(st, obs)
            for k in range(S):
                if obs[k] is not None:
                    ol, oess = orc[k].step(obs[k].t, obs[k].observation, obs[k].observation is not None)
                    assert (st[k].ll, st[k].ess, st[k].t) == (ol, oess, obs[k].t)
        outs = ff.getIntervals()
        for k in range(S):
            np.testing.assert_array_equal(st[k].particles, orc[k].particles())
            om, olo, ohi, oem, oel, oeu = orc[k].summary(0.975)
            assert (outs[k].etaIntervals.lower, outs[k].etaIntervals.upper) == (oel, oeu)
            assert [c.lower for c in outs[k].stateIntervals] == list(olo)
        datas = [[Data(float(a), float(b) if h else None) for a, b, h in zip(*cases.poisson_counts(7, seed=SEED + k, missing=0.2))] for k in range(S)]
        ll = ff.llFilter(datas)
        for k in range(S):
            assert ll[k] == orc[k].filter(*cases.poisson_counts(7, seed=SEED + k, missing=0.2))[0]
