"""Forecasts from a joint posterior sample on the GPU (cssm_pf_forecast_posterior, NativePf.forecast_posterior,
ParticleFilter.forecastPosterior).

  identity  = M = N pairs, every row the handle's parameters, x = the handle's cloud, pick = 0..N-1: every output equals cssm_pf_forecast's
              bit for bit (ties the new kernel to the path tests/test_gpu_forecast.py holds against the oracle);
  oracle    = M genuinely different rows: per row m the oracle chain of tests/test_gpu_forecast.py (OraclePf under theta_m from x[pick],
              the host twin's observation draws under theta_m's scale) over all N particles, particle i read from row pick_i's run;
  mixture   = a statistical check that shares no code: two 1-D OU parameter sets with Gaussian observations against the exact
              two-component Gaussian mixture of the OU transition, which a single-parameter forecast fails."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import pytest

import cases
from composablestatespacemodels_amd import _abi
from composablestatespacemodels_amd import formats as F
from composablestatespacemodels_amd.filter import NativePf, NativePfBatch, ParticleFilter
from composablestatespacemodels_amd.model import Data, Model, Parameters, Sde, SdeParameter, UnparamModel
from composablestatespacemodels_amd.pmmh import MetropState, pmmh_native, posterior_rows
from test_forecast_draws import build_twin
from test_forecast_posterior_host import build_pick_twin, twin_picks
from test_gpu_forecast import case, check_forecast, expected, horizon_times, ranks

pytestmark = pytest.mark.gpu

N = 4099            # odd: the last thread owns a single particle
KEY = 0x0B5E_F0CA
_dp = C.POINTER(C.c_double)
ARRAYS = ("state_mean", "state_lower", "state_upper", "eta_mean", "eta_lower", "eta_upper", "obs_mean", "obs_lower", "obs_upper", "samples")


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    return build_twin(tmp_path_factory.mktemp("twin"))


@pytest.fixture(scope="module")
def pick_twin(tmp_path_factory):
    return build_pick_twin(tmp_path_factory.mktemp("pick_twin"))


def params_of(model: Model) -> Parameters:
    return Parameters([node for _, node, _ in model.leaves])


def unparam_of(model: Model) -> UnparamModel:
    return UnparamModel([spec for spec, _, _ in model.leaves])


def posterior(model: Model, M: int, seed: int = 3, spread: float = 0.25):
    """M parameter rows around the model's (every stored value moves) and M states at t0."""
    rng = np.random.default_rng(seed)
    th0 = np.asarray(params_of(model).flattenParams())
    theta = th0 + spread * rng.standard_normal((M, th0.size))
    d = sum(sde.dimension for _, _, sde in model.leaves)
    x = 0.5 * rng.standard_normal((M, d))
    return theta, x


def expected_posterior(model, theta, x, pick, t0, times, key, twin):
    """Per row m the oracle chain over all N particles from x[pick] under theta_m; particle i from row pick_i."""
    um, p0 = unparam_of(model), params_of(model)
    states = etas = obs = None
    for m in range(theta.shape[0]):
        sm, em, om = expected(um.run(p0.withFlat(theta[m])), np.ascontiguousarray(x[pick].T), t0, times, key, twin)
        if states is None:
            states, etas, obs = sm.copy(), em.copy(), om.copy()
        sel = pick == m
        states[:, :, sel] = sm[:, :, sel]; etas[:, sel] = em[:, sel]; obs[:, sel] = om[:, sel]
    return states, etas, obs


IDENTITY_MODELS = ["c1", "c2", "c3", "linear", "negbin", "zip", "bernoulli", "studentt", "beta_scaled", "gbsg", "euler"]


@pytest.mark.parametrize("name", IDENTITY_MODELS)
def test_identity_posterior_equals_the_forecast_bit_for_bit(name):
    model, t, y, has = case(name)
    g = NativePf(model, N, cases.SEED)
    g.run(t, y, has)
    cloud = g.particles()
    theta = np.tile(np.asarray(params_of(model).flattenParams()), (N, 1))
    times = horizon_times(float(t[-1]))
    per_horizon_kib = (g.d + 2) * N * 8 / 1024
    for cap in (0, int(2 * per_horizon_kib) + 1):   # unchunked, then two horizons per chunk
        g.set_option(11, cap)
        a = g.forecast(times, KEY, 0.975, want_samples=True)
        b = g.forecast_posterior(theta, cloud.T, float(t[-1]), times, KEY, 0.975, pick=np.arange(N), want_samples=True)
        for k in ARRAYS:
            assert np.array_equal(a[k], b[k]), (name, cap, k)
        assert np.array_equal(b["pick"], np.arange(N))
    g.close()


ORACLE_MODELS = ["c1", "c2", "gbsg", "euler", "linear", "negbin", "zip", "bernoulli", "studentt", "beta_scaled", "d16"]


@pytest.mark.parametrize("name", ORACLE_MODELS)
def test_distinct_rows_match_the_oracle_per_row(name, twin, pick_twin):
    model = cases.max_dim_model() if name == "d16" else case(name)[0]
    M, t0 = 5, 3.0
    theta, x = posterior(model, M)
    if name == "beta_scaled":   # Beta's second shape is the stored scale as it is: keep it positive
        theta[:, 0] = np.abs(theta[:, 0]) + 0.1
    g = NativePf(model, N, cases.SEED)
    times = horizon_times(t0)
    r = g.forecast_posterior(theta, x, t0, times, KEY, 0.95, want_samples=True)
    pick = twin_picks(pick_twin, KEY, N, M)
    assert np.array_equal(r["pick"], pick)
    assert len(set(pick.tolist())) == M
    check_forecast(r, *expected_posterior(model, theta, x, pick.astype(np.int64), t0, times, KEY, twin), interval=0.95)
    g.close()


def _ou_moments(x0, mu, phi, sigma, dt):
    e = math.exp(-phi * dt)
    return mu + (x0 - mu) * e, sigma * sigma / (2 * phi) * (1 - e * e)


def _mixture_quantile(p, comps):
    cdf = lambda q: sum(0.5 * (1 + math.erf((q - m) / math.sqrt(2 * v))) for m, v in comps) / len(comps)
    lo, hi = -50.0, 50.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if cdf(mid) < p else (lo, mid)
    q = 0.5 * (lo + hi)
    dens = sum(math.exp(-(q - m) ** 2 / (2 * v)) / math.sqrt(2 * math.pi * v) for m, v in comps) / len(comps)
    return q, dens


def _mixture_ok(r, h, comps, n, row_mean, row_lower, row_upper, interval=0.975):
    mean = sum(m for m, _ in comps) / len(comps)
    var = sum(v + m * m for m, v in comps) / len(comps) - mean * mean
    if abs(row_mean - mean) > 5 * math.sqrt(var / n):
        return False
    for p, got in ((1 - interval, row_lower), (interval, row_upper)):
        q, dens = _mixture_quantile(p, comps)
        if abs(got - q) > 5 * math.sqrt(p * (1 - p) / n) / dens:
            return False
    return True


def test_two_parameter_sets_give_the_exact_mixture():
    n = 1 << 20
    unparam = Model.linear(Sde.ouProcess(1))
    # stored values: scale = log obs sd; OU (m0, c0 = log, phi = logit-scale, mu, sigma = log)
    sets = [(math.log(0.3), 1.5, 0.5, 0.2, 2.0, math.log(0.4)), (math.log(0.6), -1.0, 0.5, -0.4, -2.0, math.log(0.8))]
    p0 = Parameters.apply(sets[0][0], SdeParameter.ouParameterUnconstrained(0.0, 0.0, sets[0][3], sets[0][4], sets[0][5]))
    theta = np.array([[s[0], 0.0, 0.0, s[3], s[4], s[5]] for s in sets])
    assert theta.shape[1] == len(p0.flattenParams())
    x = np.array([[s[1]] for s in sets])
    t0, times = 1.0, [1.5, 2.0, 4.0]
    g = NativePf(unparam.run(p0), n, cases.SEED)
    r = g.forecast_posterior(theta, x, t0, times, KEY)
    single = g.forecast_posterior(theta[:1], x[:1], t0, times, KEY)
    for h, th in enumerate(times):
        comps, ocomps = [], []
        for s in sets:
            phi, sigma, sd = 1 / (1 + math.exp(-s[3])), math.exp(s[5]), math.exp(s[0])
            m, v = _ou_moments(s[1], s[4], phi, sigma, th - t0)
            comps.append((m, v)); ocomps.append((m, v + sd * sd))
        assert _mixture_ok(r, h, comps, n, r["state_mean"][h][0], r["state_lower"][h][0], r["state_upper"][h][0])
        assert _mixture_ok(r, h, ocomps, n, r["obs_mean"][h], r["obs_lower"][h], r["obs_upper"][h])
        assert not _mixture_ok(single, h, comps, n, single["state_mean"][h][0], single["state_lower"][h][0], single["state_upper"][h][0])
    g.close()


def test_the_handles_filter_is_untouched():
    model = cases.c2_model()
    t, y, has = cases.poisson_counts(6)
    a, b = NativePf(model, N, cases.SEED), NativePf(model, N, cases.SEED)
    la, _, ea, _ = a.run(t[:4], y[:4], has[:4])
    lb, _, eb, _ = b.run(t[:4], y[:4], has[:4])
    key_before, idx_before, cloud = a.forecast_key(), a.observation_index(), a.particles()
    theta, x = posterior(model, 7)
    a.forecast_posterior(theta, x, float(t[3]), [float(t[3]) + 1.0, float(t[3]) + 2.0], KEY, want_samples=True)
    assert np.array_equal(a.particles(), cloud) and a.forecast_key() == key_before and a.observation_index() == idx_before
    assert a.summary(0.975)[0].tolist() == b.summary(0.975)[0].tolist()
    ra, rb = a.run_more(np.ascontiguousarray(t[4:]), np.ascontiguousarray(y[4:])), b.run_more(np.ascontiguousarray(t[4:]), np.ascontiguousarray(y[4:]))
    assert ra[0] == rb[0] and np.array_equal(ra[1], rb[1]) and np.array_equal(ra[2], rb[2])
    assert np.array_equal(a.ancestors(), b.ancestors()) and np.array_equal(a.particles(), b.particles())
    a.close(); b.close()


def test_keys_reproduce_and_differ_and_chunks_do_not_matter():
    model = cases.c3_model()   # d = 9: 11 rows per horizon
    theta, x = posterior(model, 6)
    g = NativePf(model, N, cases.SEED)
    times = horizon_times(2.0)
    whole = g.forecast_posterior(theta, x, 2.0, times, KEY, want_samples=True)
    again = g.forecast_posterior(theta, x, 2.0, times, KEY, want_samples=True)
    other = g.forecast_posterior(theta, x, 2.0, times, KEY + 1, want_samples=True)
    for k in ARRAYS + ("pick",):
        assert np.array_equal(whole[k], again[k]), k
    assert not np.array_equal(whole["pick"], other["pick"])
    assert not np.array_equal(whole["samples"][:, -1], other["samples"][:, -1])
    per_horizon_kib = (g.d + 2) * N * 8 / 1024
    for cap_kib in (int(2 * per_horizon_kib) + 1, 1):   # two horizons per chunk, then one
        g.set_option(11, cap_kib)
        part = g.forecast_posterior(theta, x, 2.0, times, KEY, want_samples=True)
        for k in ARRAYS + ("pick",):
            assert np.array_equal(whole[k], part[k]), (cap_kib, k)
    g.set_option(11, 0)
    # a batch chain view lends its handle the same way
    bt = NativePfBatch(model, N, 2)
    v = bt.chain(1).forecast_posterior(theta, x, 2.0, times, KEY, want_samples=True)
    for k in ARRAYS + ("pick",):
        assert np.array_equal(whole[k], v[k]), k
    bt.close(); g.close()


@pytest.mark.slow
def test_large_cloud_final_horizon_matches_the_oracle(twin, pick_twin):
    n = 1 << 22
    model = cases.c2_model()
    M, t0 = 3, 5.0
    theta, x = posterior(model, M)
    g = NativePf(model, n, cases.SEED)
    times = t0 + np.array([0.75, 1.5, 2.25])
    g.set_option(11, 512 * 1024)   # 512 MiB: 160 MiB of keys per horizon -> chunks of 3
    r = g.forecast_posterior(theta, x, t0, times, KEY, want_samples=True)
    pick = twin_picks(pick_twin, KEY, n, M)
    assert np.array_equal(r["pick"], pick)
    states, etas, obs = expected_posterior(model, theta, x, pick.astype(np.int64), t0, times, KEY, twin)
    d = g.d
    assert np.array_equal(r["samples"][-1, :d], states[-1])
    assert np.array_equal(r["samples"][-1, d + 1], etas[-1])
    assert np.array_equal(r["samples"][-1, d + 2], obs[-1])
    (sl, su), (ol, ou) = ranks(n, 0.975)
    sa = np.sort(obs[-1])
    assert r["obs_lower"][-1] == sa[ol] and r["obs_upper"][-1] == sa[ou]
    np.testing.assert_allclose(r["state_mean"][-1], states[-1].mean(axis=1), rtol=1e-12, atol=1e-13)
    g.close()


def test_errors_name_their_row_or_cause():
    lib = _abi.load_library()
    model = cases.c2_model()
    g = NativePf(model, 256, 1)
    theta, x = posterior(model, 4)

    def rc_of(h=None, desc=None, th=theta, nt=None, xs=x, M=None, t0=1.0, times=(2.0,), pick=None, interval=0.975):
        th = np.ascontiguousarray(th, dtype=np.float64); xs = np.ascontiguousarray(xs, dtype=np.float64)
        tt = np.ascontiguousarray(times, dtype=np.float64)
        pk = None if pick is None else np.ascontiguousarray(pick, dtype=np.uint32).ctypes.data_as(C.POINTER(C.c_uint32))
        return lib.cssm_pf_forecast_posterior(h or g._h, (desc or g._desc).ptr(), th.ctypes.data_as(_dp), th.shape[1] if nt is None else nt,
                                              xs.ctypes.data_as(_dp), th.shape[0] if M is None else M, t0, tt.ctypes.data_as(_dp), len(tt), pk,
                                              KEY, interval, *([None] * 11))

    def err():
        return lib.cssm_last_error().decode()

    assert rc_of() == _abi.CSSM_OK
    assert rc_of(desc=cases.c3_model().descriptor()) == _abi.CSSM_EINVAL_DESC and "structure" in err()
    assert rc_of(nt=theta.shape[1] - 1) == _abi.CSSM_EINVAL_ARG and "n_theta" in err()
    assert rc_of(M=0) == _abi.CSSM_EINVAL_ARG and "M = 0" in err()
    bad = theta.copy(); bad[2, 3] = math.nan
    assert rc_of(th=bad) == _abi.CSSM_EINVAL_ARG and "theta row 2" in err()
    big = theta.copy(); big[1, -1] = 800.0   # sigma = exp(800): a value the model cannot use
    assert rc_of(th=big) == _abi.CSSM_EINVAL_ARG and "theta row 1" in err()
    badx = x.copy(); badx[3, 0] = math.inf
    assert rc_of(xs=badx) == _abi.CSSM_EINVAL_ARG and "x row 3" in err()
    pk = np.zeros(256, dtype=np.uint32); pk[17] = 4
    assert rc_of(pick=pk) == _abi.CSSM_EINVAL_ARG and "pick[17]" in err()
    assert rc_of(times=(0.5,)) == _abi.CSSM_EINVAL_ARG and "before t0" in err()
    assert rc_of(times=(3.0, 2.5)) == _abi.CSSM_EINVAL_ARG and "non-decreasing" in err()
    for bad_iv in (0.0, -0.1, 1.5, math.nan):
        assert rc_of(interval=bad_iv) == _abi.CSSM_EINVAL_ARG and "interval" in err()
    lg = NativePf(cases.c4_model(), 256, 1, lgcp_precision=2)
    th4, x4 = posterior(cases.c4_model(), 2)
    assert rc_of(h=lg._h, desc=lg._desc, th=th4, xs=x4) == _abi.CSSM_EINVAL_ARG and "LogGaussianCox" in err()
    h = C.c_void_p()
    _abi.check(lib.cssm_pf_create_shard(model.descriptor().ptr(), 512, 0, 256, 1, 0, None, C.byref(h)))
    try:
        assert rc_of(h=h) == _abi.CSSM_ESTATE and "sharded" in err()
    finally:
        lib.cssm_pf_destroy(h)
    with pytest.raises(ValueError):
        g.forecast_posterior(theta, x[:, :2], 1.0, [2.0])
    lg.close(); g.close()


def test_pmmh_output_forecasts_end_to_end(tmp_path):
    unparam, init = cases.c2_unparam(), cases.c2_params()
    t, y, has = cases.poisson_counts(12)
    series = [Data(float(a), float(b)) for a, b in zip(t, y)]
    iters, burn, thin = 40, 10, 3
    ll, theta, acc, last = pmmh_native(unparam, init, series, 512, 0.01, iters, seed=7)
    th, xs = posterior_rows(theta, last, burn, thin)
    t0, times, n, key = float(t[-1]), [float(t[-1]) + 1.0, float(t[-1]) + 3.0, float(t[-1]) + 6.0], 2048, 0x5EED
    outs = ParticleFilter.forecastPosterior((theta[burn::thin], last[burn::thin]), unparam, t0, times, n, 0.95, seed=key, params=init)
    assert len(outs) == len(times)
    g = NativePf(unparam.run(init.withFlat(th[0])), n)
    r = g.forecast_posterior(th, xs, t0, times, key, 0.95)
    g.close()
    for h, o in enumerate(outs):
        assert o.t == times[h] and o.obs == r["obs_mean"][h] and o.eta == r["eta_mean"][h]
        assert (o.obsIntervals.lower, o.obsIntervals.upper) == (r["obs_lower"][h], r["obs_upper"][h])
        assert np.array_equal(o.state, r["state_mean"][h])
        assert [(c.lower, c.upper) for c in o.stateIntervals] == list(zip(r["state_lower"][h], r["state_upper"][h]))
    # the same chain through the reference's JSON lines
    path = tmp_path / "chain.json"
    with open(path, "w") as f:
        for i in range(iters):
            f.write(F.metrop_state_to_json(MetropState(float(ll[i]), init.withFlat(theta[i]), last[i], int(acc[i])), t0, [1, 2]) + "\n")
    via_json = ParticleFilter.forecastPosterior(F.read_pmmh_json(str(path), burn, thin), unparam, t0, times, n, 0.95, seed=key)
    assert len(via_json) == len(outs)
    for a, b in zip(outs, via_json):
        assert F.forecast_out_csv(a) == F.forecast_out_csv(b)
        back = F.forecast_out_from_csv(F.forecast_out_csv(a))
        assert (back.t, back.obs, back.obsIntervals, back.eta, back.etaIntervals) == (a.t, a.obs, a.obsIntervals, a.eta, a.etaIntervals)
        assert np.array_equal(back.state, a.state) and back.stateIntervals == a.stateIntervals
