"""-m gpu: posterior-predictive forecasts of a whole fleet in one launch (include/cssm_pf.h: cssm_fleet_forecast_posterior;
csrc/cssm_fleet_forecast.hip: k_fleet_forecast_post, one workgroup per series).  Per series the result must be that of
cssm_pf_forecast_posterior on a handle of N particles of its own, and so of the oracle chain per posterior row plus the twin draws and
the pick twin of tests/test_gpu_forecast_posterior.py: samples, picks and order statistics bit for bit (== / assert_array_equal), the
means to check_forecast's rtol = 1e-12, atol = 1e-13 (plain fp64 sums in another order).  No series is skipped or excused."""
import ctypes as C

import numpy as np
import pytest

import cases
from composablestatespacemodels_amd import CssmError, Data, _abi
from composablestatespacemodels_amd.filter import FilterFleet, NativePf, NativePfFleet, ParticleFilter, Resampling
from composablestatespacemodels_amd.pmmh import fleet_posterior_rows, pmmh_native_fleet
from test_forecast_draws import build_twin
from test_forecast_posterior_host import build_pick_twin, twin_picks
from test_gpu_fleet import _perturbed, ragged_c2, run_key
from test_gpu_fleet_forecast import STAT, all_nan, equal_bits
from test_gpu_forecast import case, check_forecast, horizon_times
from test_gpu_forecast_posterior import ORACLE_MODELS, expected_posterior, params_of, posterior

pytestmark = pytest.mark.gpu

SEED = cases.SEED
KEY = 0xF1EE7B057E2102
MS = (1, 2, 5)


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    return build_twin(tmp_path_factory.mktemp("twin"))


@pytest.fixture(scope="module")
def pick_twin(tmp_path_factory):
    return build_pick_twin(tmp_path_factory.mktemp("pick_twin"))


def fc_key(k):
    return run_key(KEY, k)


def held_to_the_oracle(fl, k, model, post, t0, times, r, twin, pick_twin, interval=0.975):
    """series k's forecast `r` against the pick twin and the oracle chain per row + twin draws; returns the expected arrays"""
    assert r["rc"] == 0, (k, r["rc"])
    theta, x = post
    pick = twin_picks(pick_twin, r["key"], fl.n, theta.shape[0])
    np.testing.assert_array_equal(r["pick"], pick)
    exp = expected_posterior(model, theta, x, pick.astype(np.int64), float(t0), np.asarray(times, dtype=np.float64), r["key"], twin)
    assert r["state_mean"].shape == (len(times), fl.d) and r["samples"].shape == (len(times), fl.d + 3, fl.n)
    check_forecast(r, *exp, interval=interval)
    return exp


def equals_a_handle_of_its_own(model, n, seed, post, t0, times, key, interval, r, pick=None):
    with NativePf(model, n, seed) as g:
        own = g.forecast_posterior(post[0], post[1], float(t0), times, key, interval, pick=pick, want_samples=True)
    np.testing.assert_array_equal(r["samples"], own["samples"])
    np.testing.assert_array_equal(r["pick"], own["pick"])
    for name in STAT:
        if name.endswith("_mean"):
            np.testing.assert_allclose(r[name], own[name], rtol=1e-12, atol=1e-13, err_msg=name)
        else:
            np.testing.assert_array_equal(r[name], own[name], err_msg=name)


# 1 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 63, 100, _abi.FLEET_MAX_N])
def test_ragged_fleet_posterior_forecasts_equal_the_oracle_and_handles_of_their_own(n, twin, pick_twin):
    """clamped ranks (1), a pair (2), an odd sub-wave cloud (63), padding to a power of two (100), the LDS maximum (4096); M_k cycling
    through 1, 2, 5; 1 .. 5 horizons per series (equal times: a dt = 0 step), none for every sixth; a fleet that was never initialised"""
    S = 24
    models, seeds, datas = ragged_c2(S)
    t0 = [float(d[0][-1]) for d in datas]
    times = [horizon_times(t0[k])[:1 + k % 5] if k % 6 != 5 else (None if k % 12 == 5 else np.zeros(0)) for k in range(S)]
    keys = [fc_key(k) for k in range(S)]
    post = [posterior(models[k], MS[k % 3], seed=3 + k) for k in range(S)]
    with NativePfFleet(models[0], n, S) as fl:
        fl.set_params(models); fl.reseed(seeds)
        exp, first = {}, {}
        for interval, how in ((0.975, 1), (0.5, 2), (0.975, 2), (0.5, 1)):      # CSSM_OPT_FLEET_SELECT: the bitonic sort, the radix select
            fl.set_option(12, how)
            rs = fl.forecast_posterior(post, t0, times, keys, interval, want_samples=True)
            assert len(rs) == S
            if (interval, how) in ((0.975, 2), (0.5, 1)):      # the other way to the same order statistics: the same bits
                for k in range(S):
                    equal_bits(rs[k], first[interval][k])
                    np.testing.assert_array_equal(rs[k]["pick"], first[interval][k]["pick"])
                continue
            first[interval] = rs
            for k in range(S):
                assert rs[k]["key"] == keys[k]
                if k % 6 == 5:                                 # no horizons: nothing but the picks
                    assert rs[k]["rc"] == 0 and rs[k]["state_mean"].shape == (0, fl.d) and rs[k]["samples"].shape[0] == 0
                    np.testing.assert_array_equal(rs[k]["pick"], twin_picks(pick_twin, keys[k], n, MS[k % 3]))
                    continue
                if k not in exp:
                    exp[k] = held_to_the_oracle(fl, k, models[k], post[k], t0[k], times[k], rs[k], twin, pick_twin, interval)
                else:
                    check_forecast(rs[k], *exp[k], interval=interval)
                if n in (100, _abi.FLEET_MAX_N):
                    equals_a_handle_of_its_own(models[k], n, seeds[k], post[k], t0[k], times[k], keys[k], interval, rs[k])


# 2 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [m for m in ORACLE_MODELS if m != "d16"])
def test_every_served_observation_model(name, twin, pick_twin):
    S, n, M, t0 = 4, 100, 5, 3.0
    model = case(name)[0]
    post = [posterior(model, M, seed=3 + k) for k in range(S)]
    if name == "beta_scaled":   # Beta's second shape is the stored scale as it is: keep it positive
        for th, _ in post:
            th[:, 0] = np.abs(th[:, 0]) + 0.1
    times = [horizon_times(t0)] * S
    with NativePfFleet(model, n, S) as fl:
        rs = fl.forecast_posterior(post, t0, times, [fc_key(k) for k in range(S)], 0.95, want_samples=True)
        for k in range(S):
            held_to_the_oracle(fl, k, model, post[k], t0, times[k], rs[k], twin, pick_twin, 0.95)
            assert np.all(np.isfinite(rs[k]["samples"][:, fl.d]))      # the gamma row: f(x, t)


# 3 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", list(range(1, 17)))
def test_every_latent_dimension(d):
    """d = 8, 9 and 16: where the register-resident and the row-read parameter paths of the single handle and of the fleet meet"""
    model = cases.dim_model(d)
    S, n, M, t0 = 3, 100, 3, 2.0
    seeds = [SEED + 17 * k for k in range(S)]
    post = [posterior(model, M, seed=5 + k) for k in range(S)]
    times = [horizon_times(t0)[1:4]] * S
    with NativePfFleet(model, n, S) as fl:
        assert fl.d == d
        fl.reseed(seeds)
        rs = fl.forecast_posterior(post, t0, times, [fc_key(k) for k in range(S)], 0.9, want_samples=True)
        for k in range(S):
            assert rs[k]["rc"] == 0 and len(set(rs[k]["pick"].tolist())) == M
            equals_a_handle_of_its_own(model, n, seeds[k], post[k], t0, times[k], fc_key(k), 0.9, rs[k])


# 4 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [63, 100])
def test_identity_posterior_equals_the_fleet_forecast_bit_for_bit(n):
    """theta = the series' own parameters N times, x = its cloud, pick = 0 .. N-1, t0 = its clock: cssm_fleet_forecast's bits"""
    S = 8
    models, seeds, datas = ragged_c2(S)
    clock = [float(d[0][-1]) for d in datas]
    times = [horizon_times(clock[k]) for k in range(S)]
    keys = [fc_key(k) for k in range(S)]
    with NativePfFleet(models[0], n, S) as fl:
        fl.set_params(models); fl.reseed(seeds)
        _, _, _, rc = fl.ll_filter(datas)
        assert not rc.any(), rc
        assert {fl.observation_index(k) & 1 for k in range(S)} == {0, 1}                  # clouds in both buffers
        a = fl.forecast(times, keys, 0.9, want_samples=True)
        post = [(np.tile(np.asarray(params_of(models[k]).flattenParams()), (n, 1)), fl.particles(k).T) for k in range(S)]
        b = fl.forecast_posterior(post, clock, times, keys, 0.9, picks=np.tile(np.arange(n), (S, 1)), want_samples=True)
        for k in range(S):
            assert a[k]["rc"] == 0 and b[k]["rc"] == 0
            equal_bits(a[k], b[k])
            np.testing.assert_array_equal(b[k]["pick"], np.arange(n))


# 5 ------------------------------------------------------------------------------------------------------------------------------
def test_given_picks_and_drawn_picks(pick_twin):
    S, n = 5, 100
    models, seeds, _ = ragged_c2(S)
    Ms = [3, 1, 4, 2, 6]
    post = [posterior(models[k], Ms[k], seed=11 + k) for k in range(S)]
    times = [[1.5, 2.0], None, [1.25], np.zeros(0), [4.0]]                                # series 1 and 3: no horizons, M_k > 0
    keys = [fc_key(k) for k in range(S)]
    rng = np.random.default_rng(4)
    picks = np.array([rng.integers(0, Ms[k], n) for k in range(S)])
    with NativePfFleet(models[0], n, S) as fl:
        fl.set_params(models)
        given = fl.forecast_posterior(post, 1.0, times, keys, picks=picks, want_samples=True)
        drawn = fl.forecast_posterior(post, 1.0, times, keys, want_samples=True)
        for k in range(S):
            assert given[k]["rc"] == 0 and drawn[k]["rc"] == 0
            np.testing.assert_array_equal(given[k]["pick"], picks[k])
            np.testing.assert_array_equal(drawn[k]["pick"], twin_picks(pick_twin, keys[k], n, Ms[k]))
        for k in (0, 2, 4):
            equals_a_handle_of_its_own(models[k], n, 1, post[k], 1.0, times[k], keys[k], 0.975, given[k], pick=picks[k])
            # the caller's picks are the drawn ones: the drawn forecast
            again = fl.forecast_posterior(post, 1.0, times, keys, picks=np.array([r["pick"] for r in drawn]), want_samples=True)
            equal_bits(again[k], drawn[k])


# 6 ------------------------------------------------------------------------------------------------------------------------------
def test_the_fleet_is_untouched():
    """The states between horizons live in the series' state buffer that does not hold its cloud: after a posterior forecast everything
    the fleet holds reads as before and its next step and forecast are those of a fleet that never ran one -- whichever buffer a
    series' cloud is in.  A fleet without any cloud serves the call with the same bits."""
    model = cases.c2_model()
    S, n = 6, 100
    seeds = [run_key(SEED, k) for k in range(S)]
    ys = [cases.poisson_counts(6, seed=SEED + k)[1] for k in range(S)]
    post = [posterior(model, MS[k % 3], seed=21 + k) for k in range(S)]
    with NativePfFleet(model, n, S) as fl, NativePfFleet(model, n, S) as ref, NativePfFleet(model, n, S) as fresh:
        clock = np.array([0.25 * k for k in range(S)])
        for f in (fl, ref):
            f.reseed(seeds)
            f.init(clock)
        for r in range(3):                                     # series k has seen 3, 2, 1, 3, 2, 1 observations: both parities
            active = np.array([r < 3 - k % 3 for k in range(S)], dtype=np.uint8)
            clock = clock + 0.5 * active
            y = np.array([ys[k][r] for k in range(S)])
            for f in (fl, ref):
                assert not f.step(clock, y, None, active)[2].any()
        assert [fl.observation_index(k) for k in range(S)] == [3 - k % 3 for k in range(S)]
        times = [horizon_times(clock[k]) for k in range(S)]
        keys = [fc_key(k) for k in range(S)]
        runs = [fl.forecast_posterior(post, clock, times, keys, 0.975, want_samples=ws) for ws in (False, True)]
        assert not any(r["rc"] for rs in runs for r in rs)
        unborn = fresh.forecast_posterior(post, clock, times, keys, 0.975, want_samples=True)       # never initialised: no CSSM_ESTATE
        for k in range(S):
            equal_bits(unborn[k], runs[1][k])
            np.testing.assert_array_equal(unborn[k]["pick"], runs[1][k]["pick"])
            for name in STAT:
                np.testing.assert_array_equal(runs[0][k][name], runs[1][k][name])
            np.testing.assert_array_equal(fl.particles(k), ref.particles(k))
            np.testing.assert_array_equal(fl.ancestors(k), ref.ancestors(k))
            assert fl.observation_index(k) == ref.observation_index(k) and fl.forecast_key(k) == ref.forecast_key(k)
        for a, b in zip(fl.summary(0.9), ref.summary(0.9)):
            np.testing.assert_array_equal(a, b)
        clock = clock + 0.75
        y = np.array([ys[k][4] for k in range(S)])
        for a, b in zip(fl.step(clock, y), ref.step(clock, y)):
            np.testing.assert_array_equal(a, b)
        times = [horizon_times(clock[k]) for k in range(S)]
        fa, fb = fl.forecast(times, keys, 0.9, want_samples=True), ref.forecast(times, keys, 0.9, want_samples=True)
        for k in range(S):
            np.testing.assert_array_equal(fl.particles(k), ref.particles(k))
            np.testing.assert_array_equal(fl.ancestors(k), ref.ancestors(k))
            assert fa[k]["rc"] == 0
            equal_bits(fa[k], fb[k])


# 7 ------------------------------------------------------------------------------------------------------------------------------
def test_one_series_errors_are_its_own():
    model = cases.c2_model()
    S, n, t0 = 4, 100, 1.0
    post = [posterior(model, 4, seed=31 + k) for k in range(S)]
    times = [horizon_times(t0)[:3] for _ in range(S)]
    keys = [fc_key(k) for k in range(S)]
    nt = post[0][0].shape[1]

    def spoilt(**kw):
        """series 1's arguments with one fault: (posteriors, times, picks)"""
        th, x = post[1][0].copy(), post[1][1].copy()
        ts, pk = [np.array(v) for v in times], None
        if "M0" in kw: th, x = th[:0], x[:0]
        if "theta" in kw: th[kw["theta"]] = kw["value"]
        if "x" in kw: x[kw["x"]] = np.nan
        if "times" in kw: ts[1] = np.array(kw["times"])
        if "pick" in kw:
            pk = np.zeros((S, n), dtype=np.int64); pk[1, 17] = 4
        return [post[0], (th, x), post[2], post[3]], ts, pk

    with NativePfFleet(model, n, S) as fl:
        clean = fl.forecast_posterior(post, t0, times, keys, 0.975, want_samples=True)
        clean_picked = fl.forecast_posterior(post, t0, times, keys, 0.975, picks=np.zeros((S, n), dtype=np.int64), want_samples=True)
        assert not any(r["rc"] for r in clean + clean_picked)
        faults = [(dict(M0=True), "series 1: the posterior sample is empty"), (dict(theta=(2, 3), value=np.nan), "series 1: theta row 2"),
                  (dict(theta=(1, -1), value=800.0), "series 1: theta row 1"),            # sigma = exp(800): a value the model cannot use
                  (dict(x=(3, 0)), "series 1: x row 3"), (dict(pick=True), "series 1: pick[17]"),
                  (dict(times=[t0 - 0.5, t0 + 1.0]), "series 1: t[0] is before t0"), (dict(times=[t0 + 1.0, t0 + 0.5]), "series 1: t must be non-decreasing"),
                  (dict(times=[t0 + 1.0, np.inf]), "series 1: t[1] is not finite")]
        for kw, words in faults:
            ps, ts, pk = spoilt(**kw)
            rs = fl.forecast_posterior(ps, t0, ts, keys, 0.975, picks=pk, want_samples=True)
            assert words in fl.lib.cssm_last_error().decode(), (kw, fl.lib.cssm_last_error())
            assert [r["rc"] for r in rs] == [0, _abi.CSSM_EINVAL_ARG, 0, 0], kw
            assert all_nan(rs[1]) and rs[1]["samples"].shape == (len(ts[1]), fl.d + 3, n), kw
            for k in (0, 2, 3):
                equal_bits(rs[k], (clean_picked if pk is not None else clean)[k])
        # call-level refusals carry a message and change nothing
        p = lambda arr, ty: arr.ctypes.data_as(C.POINTER(ty))
        moff, theta, x = fl.pack_posteriors(post)
        off, tt = fl.pack_times(times)
        t0s = np.full(S, t0); ky = np.array(keys, dtype=np.uint64); rc = np.zeros(S, dtype=np.int32)

        def call(f=fl._h, desc=fl._desc, moff=moff, nth=nt, off=off, interval=0.975, null=None):
            a = [f, desc.ptr(), p(moff, C.c_uint64), p(theta, C.c_double), nth, p(x, C.c_double), p(t0s, C.c_double), p(off, C.c_uint64),
                 p(tt, C.c_double), None, p(ky, C.c_uint64), interval, *([None] * 11), p(rc, C.c_int)]
            if null is not None:
                a[null] = None
            return fl.lib.cssm_fleet_forecast_posterior(*a), fl.lib.cssm_last_error().decode()

        assert call()[0] == _abi.CSSM_OK
        for null in (0, 1, 2, 3, 5, 6, 7, 8, 10, 23):
            code, msg = call(null=null)
            assert code == _abi.CSSM_EINVAL_ARG and "null" in msg, null
        bad = moff.copy(); bad[0] = 1
        assert call(moff=bad) == (_abi.CSSM_EINVAL_ARG, "moff[0] must be 0")
        bad = off.copy(); bad[0] = 1
        assert call(off=bad) == (_abi.CSSM_EINVAL_ARG, "off[0] must be 0")
        bad = moff.copy(); bad[2] = bad[1] - 1
        code, msg = call(moff=bad)
        assert code == _abi.CSSM_EINVAL_ARG and "moff must be non-decreasing" in msg
        bad = off.copy(); bad[2] = bad[1] - 1
        code, msg = call(off=bad)
        assert code == _abi.CSSM_EINVAL_ARG and "off must be non-decreasing" in msg
        for interval in (0.0, 1.5, np.nan):
            code, msg = call(interval=interval)
            assert code == _abi.CSSM_EINVAL_ARG and "interval" in msg
        code, msg = call(nth=nt - 1)
        assert code == _abi.CSSM_EINVAL_ARG and "n_theta" in msg
        code, msg = call(desc=cases.c3_model().descriptor())                              # another structure
        assert code == _abi.CSSM_EINVAL_DESC and "structure" in msg
        code, msg = call(desc=cases.c4_model().descriptor())                              # LGCP: never a fleet's structure
        assert code == _abi.CSSM_EINVAL_DESC and msg
        with pytest.raises(CssmError) as e:
            fl.forecast_posterior(post, t0, times, keys, 1.5)
        assert e.value.code == _abi.CSSM_EINVAL_ARG and "interval" in str(e.value)
        nothing = fl.forecast_posterior([None] * S, t0, [None] * S, keys)                 # nobody has rows or horizons: nothing refused
        assert [r["rc"] for r in nothing] == [0] * S and all(r["state_mean"].shape == (0, fl.d) for r in nothing)
        again = fl.forecast_posterior(post, t0, times, keys, 0.975, want_samples=True)    # still usable
        for k in range(S):
            assert again[k]["rc"] == 0
            equal_bits(again[k], clean[k])
    # a model without the scale its observation needs: every series with a posterior is refused -- with or without horizons, as the
    # single handle refuses it for any H --, the call succeeds, the message stays
    beta = cases.literal_case("beta", 4)[0]
    with NativePfFleet(beta, n, 3) as fl:
        pb = [posterior(beta, 2, seed=0), posterior(beta, 2, seed=1), None]
        rs = fl.forecast_posterior(pb, 0.0, [[1.0], None, None], [1, 2, 3], want_samples=True)
        assert [r["rc"] for r in rs] == [_abi.CSSM_EINVAL_ARG, _abi.CSSM_EINVAL_ARG, 0] and all_nan(rs[0])
        assert not rs[0]["pick"].any() and not rs[1]["pick"].any()
        msg = fl.lib.cssm_last_error()
        assert b"series 0" in msg and b"Must provide shape parameter for Beta Model" in msg


# 8 ------------------------------------------------------------------------------------------------------------------------------
def test_more_blocks_than_the_gpu_holds(twin, pick_twin):
    model = cases.c1_model()
    S, n, H, M = 2500, 64, 3, 2
    keys = [run_key(SEED, k) for k in range(S)]
    rng = np.random.default_rng(8)
    th0 = np.asarray(params_of(model).flattenParams())
    post = [(th0 + 0.25 * rng.standard_normal((M, th0.size)), 0.5 * rng.standard_normal((M, 1))) for _ in range(S)]
    times = [horizon_times(2.0)[:H]] * S
    with NativePfFleet(model, n, S) as fl:
        rs = fl.forecast_posterior(post, 2.0, times, keys, 0.975, want_samples=True)
        assert not any(r["rc"] for r in rs)
        for k in (0, 1, 255, 256, 1023, 2048, S - 1):
            held_to_the_oracle(fl, k, model, post[k], 2.0, times[k], rs[k], twin, pick_twin)
        stats = fl.forecast_posterior(post, 2.0, times, keys)  # without samples: the same statistics
        for k in range(0, S, 97):
            for name in STAT:
                np.testing.assert_array_equal(stats[k][name], rs[k][name])
            np.testing.assert_array_equal(stats[k]["pick"], rs[k]["pick"])


# 9 ------------------------------------------------------------------------------------------------------------------------------
def test_samples_in_chunks_of_series_equal_the_whole():
    S, n = 12, 100
    models, seeds, _ = ragged_c2(S)
    post = [posterior(models[k], MS[k % 3], seed=41 + k) for k in range(S)]
    times = [horizon_times(1.0)[:k % 6] for k in range(S)]     # 0 .. 5 horizons
    keys = [fc_key(k) for k in range(S)]
    with NativePfFleet(models[0], n, S) as fl:
        fl.set_params(models)
        whole = fl.forecast_posterior(post, 1.0, times, keys, want_samples=True)
        row_kib = (fl.d + 3) * n * 8 / 1024
        for cap_kib in (int(7 * row_kib) + 1, 1):              # two series or so per chunk; one series per chunk (it is never split)
            fl.set_option(11, cap_kib)
            part = fl.forecast_posterior(post, 1.0, times, keys, want_samples=True)
            for k in range(S):
                assert part[k]["rc"] == 0
                equal_bits(part[k], whole[k])
                np.testing.assert_array_equal(part[k]["pick"], whole[k]["pick"])
        fl.set_option(11, 0)


# 10 -----------------------------------------------------------------------------------------------------------------------------
def test_fleet_pmmh_output_forecasts_end_to_end():
    um = cases.c2_unparam()
    S, n, iters = 3, 100, 12
    inits = [_perturbed(cases.c2_params, k) for k in range(S)]
    t, y, _ = cases.poisson_counts(8)
    series = [Data(float(a), float(b)) for a, b in zip(t, y)]
    _, theta, _, last = pmmh_native_fleet(um, inits, series, n, 0.01, iters, seeds=[7, 8, 9])
    rows = fleet_posterior_rows(theta, last, burn_in=2, thin=2)
    assert len(rows) == S and rows[0][0].shape[0] == 5
    t0 = float(t[-1])
    times = [[t0 + 1.0, t0 + 3.0], [t0 + 0.5], [t0 + 1.0, t0 + 1.0, t0 + 6.0]]
    lib = _abi.load_library()
    with FilterFleet([um.run(p) for p in inits], Resampling.systematicResampling, n, seed=SEED) as ff:
        default_keys = [int(lib.cssm_pf_run_key(run_key(SEED, k), 1 << 63)) for k in range(S)]
        for seed, key_of in ((0x5EED, lambda k: 0x5EED), (None, lambda k: default_keys[k])):
            outs = ff.forecastPosterior(rows, t0, times, 0.95, seed=seed, params=inits[0])
            assert [len(o) for o in outs] == [len(v) for v in times]
            for k in range(S):
                want = ParticleFilter.forecastPosterior(rows[k], um, t0, times[k], n, 0.95, seed=key_of(k), params=inits[0])
                for a, b in zip(outs[k], want):
                    assert (a.t, a.obsIntervals, a.etaIntervals, a.stateIntervals) == (b.t, b.obsIntervals, b.etaIntervals, b.stateIntervals)
                    np.testing.assert_allclose([a.obs, a.eta], [b.obs, b.eta], rtol=1e-12, atol=1e-13)
                    np.testing.assert_allclose(a.state, b.state, rtol=1e-12, atol=1e-13)
        with pytest.raises(CssmError, match="series 1"):
            ff.forecastPosterior(rows, t0, [times[0], [t0 - 1.0], times[2]], 0.95, params=inits[0])
