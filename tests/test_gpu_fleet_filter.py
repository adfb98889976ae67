"""-m gpu: `filter` of a fleet (cssm_fleet_filter): every series' sampled path recorded by its own workgroup inside the one launch.  Per
series the path is the oracle's and a handle's own, bit for bit, and everything else is what cssm_fleet_ll_filter leaves: every comparison
is == / assert_array_equal, no series is skipped or excused."""
import numpy as np
import pytest

import cases
from composablestatespacemodels_amd import Data, _abi
from composablestatespacemodels_amd.filter import Filter, FilterFleet, NativePf, NativePfFleet, Resampling
from oracle import oracle
from test_gpu_fleet import SEED, ragged_c2, run_key

pytestmark = pytest.mark.gpu


def oracle_filter(model, n, seed, data):
    o = oracle.OraclePf(model.descriptor(), n, seed)
    return o, o.filter(*data, want_path=True)


def assert_filter_equals_oracle(res, k, model, n, seed, data):
    ll, ll_t, ess_t, paths, last, rc = res
    assert rc[k] == 0
    o, (ol, oll_t, oess_t, opath) = oracle_filter(model, n, seed, data)
    assert ll[k] == ol, (k, n, ll[k], ol)
    np.testing.assert_array_equal(ll_t[k], oll_t)
    np.testing.assert_array_equal(ess_t[k], oess_t)
    assert paths[k].shape == opath.shape == (len(data[0]) + 1, o.d)
    np.testing.assert_array_equal(paths[k], opath)
    np.testing.assert_array_equal(last[k], opath[-1])
    return o


# 1 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 63, 100, 1000, _abi.FLEET_MAX_N])
def test_ragged_fleet_paths_equal_the_oracle_and_handles_of_their_own(n):
    S = 24
    models, seeds, datas = ragged_c2(S)
    with NativePfFleet(models[0], n, S) as fl, NativePfFleet(models[0], n, S) as plain:
        fl.set_params(models); plain.set_params(models)
        for sd in (seeds, seeds[1:] + seeds[:1]):            # the same fleet again with the seeds rotated by one (buffers reused)
            fl.reseed(sd); plain.reseed(sd)
            res = fl.filter(datas)
            ll, ll_t, ess_t, paths, last, rc = res
            pl, pll_t, pess_t, prc = plain.ll_filter(datas)
            assert not rc.any() and not prc.any(), (rc, prc)
            np.testing.assert_array_equal(ll, pl)
            for k in range(S):
                o = assert_filter_equals_oracle(res, k, models[k], n, sd[k], datas[k])
                np.testing.assert_array_equal(ll_t[k], pll_t[k])
                np.testing.assert_array_equal(ess_t[k], pess_t[k])
                for a in (fl, plain):
                    np.testing.assert_array_equal(a.particles(k), o.particles())
                    np.testing.assert_array_equal(a.ancestors(k), o.ancestors())
                assert fl.observation_index(k) == plain.observation_index(k) == len(datas[k][0])
                if n in (100, _abi.FLEET_MAX_N):
                    with NativePf(models[k], n, sd[k]) as g:
                        gl, _, _, gpath = g.run(*datas[k], want_path=True)
                        assert gl == ll[k]
                        np.testing.assert_array_equal(paths[k], gpath)


# 2 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", list(range(1, 17)))
def test_every_latent_dimension(d):
    model = cases.dim_model(d)
    S, n = 3, 257
    seeds = [SEED + 17 * k for k in range(S)]
    datas = [cases.poisson_counts(6, seed=SEED + k) for k in range(S)]
    with NativePfFleet(model, n, S) as fl:
        fl.reseed(seeds)
        res = fl.filter(datas)
        assert not res[5].any()
        for k in range(S):
            assert_filter_equals_oracle(res, k, model, n, seeds[k], datas[k])


@pytest.mark.parametrize("name", ["linear", "negbin"])
def test_a_gaussian_observation_and_one_with_a_scale(name):
    model = cases.linear_model() if name == "linear" else cases.literal_case("negbin", 12)[0]
    gen = cases.gaussian_series if name == "linear" else cases.poisson_counts
    S, n, T = 5, 1000, 12
    seeds = [SEED + 17 * k for k in range(S)]
    datas = [gen(T, seed=SEED + k) for k in range(S)]
    with NativePfFleet(model, n, S) as fl:
        fl.reseed(seeds)
        res = fl.filter(datas)
        assert not res[5].any()
        for k in range(S):
            assert_filter_equals_oracle(res, k, model, n, seeds[k], datas[k])


# 3 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [100, 1000])
def test_last_rows_alone_equal_the_last_rows_of_the_paths(n):
    S = 24
    models, seeds, datas = ragged_c2(S)
    with NativePfFleet(models[0], n, S) as fl:
        fl.set_params(models); fl.reseed(seeds)
        ll, ll_t, ess_t, paths, last, rc = fl.filter(datas)
        ll2, ll_t2, ess_t2, none, last2, rc2 = fl.filter(datas, want_path=False)
        assert none is None and not rc.any() and not rc2.any()
        np.testing.assert_array_equal(ll2, ll)
        np.testing.assert_array_equal(last2, last)
        np.testing.assert_array_equal(last2, np.stack([p[-1] for p in paths]))
        for k in range(S):
            np.testing.assert_array_equal(ll_t2[k], ll_t[k])
            np.testing.assert_array_equal(ess_t2[k], ess_t[k])
        assert np.all(np.isfinite(last2))


# 4 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [100, 1000])
def test_one_series_fails_and_the_others_do_not_notice(n):
    """test_gpu_fleet's failing series: y = 1e200 at observation 3 of series 2.  Its rows 0 .. 3 were recorded before that observation
    was weighed; from row 4 on, and in `last`, it reads NaN."""
    model = cases.linear_model()
    S = 4
    seeds = [SEED + 17 * k for k in range(S)]
    datas = [cases.gaussian_series(8, seed=SEED + k) for k in range(S)]
    bad = datas[2][1].copy(); bad[3] = 1e200
    datas[2] = (datas[2][0], bad, datas[2][2])
    with NativePfFleet(model, n, S) as fl:
        fl.reseed(seeds)
        for want_path in (True, False):
            res = fl.filter(datas, want_path=want_path)
            ll, ll_t, ess_t, paths, last, rc = res
            assert list(rc) == [0, 0, _abi.CSSM_ENONFINITE, 0]
            assert np.all(np.isnan(last[2])) and np.isnan(ll[2])
            for k in (0, 1, 3):
                o, (ol, _, _, opath) = oracle_filter(model, n, seeds[k], datas[k])
                assert ll[k] == ol
                np.testing.assert_array_equal(last[k], opath[-1])
                if want_path:
                    assert_filter_equals_oracle(res, k, model, n, seeds[k], datas[k])
                np.testing.assert_array_equal(fl.particles(k), o.particles())
            if not want_path:
                continue
            o = oracle.OraclePf(model.descriptor(), n, seeds[2])
            with pytest.raises(oracle.OracleError):
                o.filter(*datas[2])                          # (the premise: the oracle cannot weigh that observation either)
            pick = lambda row: int(oracle.lib().oracle_c_pick(seeds[2], row, n))
            o.init(datas[2][0][0])
            np.testing.assert_array_equal(paths[2][0], o.particles()[:, pick(0)])
            for s in range(3):
                o.step(datas[2][0][s], datas[2][1][s], True)
                np.testing.assert_array_equal(paths[2][s + 1], o.particles()[:, pick(s + 1)])
                np.testing.assert_array_equal(paths[2][s + 1], o.proposed()[:, o.ancestors()[pick(s + 1)]])
            assert paths[2].shape == (9, 1) and np.all(np.isnan(paths[2][4:]))


# 5 ------------------------------------------------------------------------------------------------------------------------------
def test_filter_then_step_equals_handles_of_their_own():
    S, n = 6, 1000
    models, seeds, datas = ragged_c2(S)
    nxt = [cases.poisson_counts(2, seed=SEED + 50 + k)[1] for k in range(S)]
    with NativePfFleet(models[0], n, S) as fl:
        fl.set_params(models); fl.reseed(seeds)
        ll, _, _, paths, _, rc = fl.filter(datas)
        assert not rc.any()
        hs = [NativePf(models[k], n, seeds[k]) for k in range(S)]
        try:
            for k in range(S):
                gl, _, _, gpath = hs[k].run(*datas[k], want_path=True)
                assert gl == ll[k]
                np.testing.assert_array_equal(paths[k], gpath)
            clock = np.array([datas[k][0][-1] for k in range(S)])
            for r in range(2):
                clock = clock + 0.5 * (1 + r)
                y = np.array([nxt[k][r] for k in range(S)])
                has = np.array([(r + k) % 3 != 0 for k in range(S)], dtype=np.uint8)
                l2, e2, rc = fl.step(clock, y, has)
                assert not rc.any()
                for k in range(S):
                    gl, gess = hs[k].step(float(clock[k]), float(y[k]), bool(has[k]))
                    assert (l2[k], e2[k]) == (gl, gess), (r, k)
            for k in range(S):
                np.testing.assert_array_equal(fl.particles(k), hs[k].particles())
                np.testing.assert_array_equal(fl.ancestors(k), hs[k].ancestors())
        finally:
            for h in hs:
                h.close()


# 6 ------------------------------------------------------------------------------------------------------------------------------
def test_scale_more_blocks_than_the_gpu_holds():
    model = cases.c1_model()
    S, n, T = 2000, 100, 8
    keys = [run_key(SEED, k) for k in range(S)]
    datas = [cases.poisson_counts(T, seed=SEED + k, missing=(0, .2)[k % 2]) for k in range(S)]
    with NativePfFleet(model, n, S) as fl:
        fl.reseed(keys)
        res = fl.filter(datas)
        assert not res[5].any()
        np.testing.assert_array_equal(res[4], np.stack([p[-1] for p in res[3]]))
        for k in range(0, S, 125):                            # 16 of them
            assert_filter_equals_oracle(res, k, model, n, keys[k], datas[k])


def test_filter_fleet_returns_what_filter_returns_per_series():
    S, n = 4, 500
    models, _, arrs = ragged_c2(S)
    datas = [[Data(float(a), float(b) if h else None) for a, b, h in zip(*arrs[k])] for k in range(S)]
    with FilterFleet(models, Resampling.systematicResampling, n, seed=SEED) as ff:
        outs = ff.filter(datas)
        assert len(outs) == S
        for k in range(S):
            ll, path = Filter(models[k], Resampling.systematicResampling, seed=run_key(SEED, k)).filter(datas[k], n)
            fll, fpath = outs[k]
            assert fll == ll and len(fpath) == len(path) == len(datas[k]) + 1
            assert fpath[0].time == min(d.t for d in datas[k])
            for a, b in zip(fpath, path):
                assert a.time == b.time
                np.testing.assert_array_equal(a.state, b.state)
