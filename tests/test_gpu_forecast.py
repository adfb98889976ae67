"""Forecasts from the filtered cloud on the GPU (cssm_pf_forecast, cssm_obs_draw, ParticleFilter.forecast / getMeanForecast /
getForecast), held against the oracle's state chain bit for bit:

  states   = OraclePf(desc, n, key): init_from, set_particles(cloud), then propagate_only(t_h) / proposed() per horizon -- what an
             unweighted filter step with seed `key` and observation index h draws;
  eta      = the oracle's eta() of those states at t_h;
  obs      = the host twin of include/cssm_obs_draws.h (tests/cpp/obs_draw_twin.c) on those etas at (key, particle, h);
  summaries= numpy's sort of those arrays at the reference's ranks, means to 1e-12."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import pytest

import cases
from composablestatespacemodels_amd import _abi
from composablestatespacemodels_amd import formats as F
from composablestatespacemodels_amd.filter import (Filter, FilterInit, NativePf, NativePfBatch, ParticleFilter, Resampling)
from composablestatespacemodels_amd.model import Data, Model, Parameters, Sde, SdeParameter
from oracle import oracle
from test_forecast_draws import build_twin

pytestmark = pytest.mark.gpu

N = 4099            # odd: the last thread owns a single particle
KEY = 0xF0CA57
STEPS = 4
_dp = C.POINTER(C.c_double)


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    return build_twin(tmp_path_factory.mktemp("twin"))


def beta_scaled_model():
    p = Parameters.apply(0.8, SdeParameter.ouParameter(0.5, 0.2, 0.2, 0.5, 0.2))
    return Model.beta(Sde.ouProcess(1)).run(p)


def case(name, T=STEPS):
    if name == "beta_scaled":
        return (beta_scaled_model(),) + tuple(cases.unit_interval_series(T))
    return cases.literal_case(name, T)


def horizon_times(t0):
    return t0 + np.array([0.5, 0.5, 1.75, 3.0, 7.25])   # dt = 0.5, 0 (equal times), 1.25, 1.25, 4.25


def expected(model, cloud, t_cloud, times, key, twin, interval=0.975):
    """(states[H, d, n], eta[H, n], obs[H, n]) from the oracle chain and the twin draws."""
    desc = model.descriptor()
    d, n = cloud.shape
    o = oracle.OraclePf(desc, n, key)
    o.init_from(t_cloud, np.zeros(d))
    o.set_particles(cloud)
    L = desc.leaf_array[0]
    kind, df = desc.desc.obs_kind, desc.desc.obs_df
    states, etas, obs = [], [], []
    for h, th in enumerate(times):
        o.propagate_only(float(th), None, False)
        x = o.proposed()
        o.set_particles(x)
        e = o.eta()
        out = np.zeros(n)
        assert twin.twin_obs_draw(kind, e.ctypes.data_as(_dp), n, L.has_scale, L.scale, df, key, h, out.ctypes.data_as(_dp)) == 0
        states.append(x); etas.append(e); obs.append(out)
    return np.array(states), np.array(etas), np.array(obs)


def ranks(n, interval):
    idx = int(math.floor(interval * n))
    c = lambda r: min(max(r, 0), n - 1)
    return (c(n - idx - 1), c(idx - 1)), (c(n - idx), c(idx))


def check_forecast(r, states, etas, obs, interval=0.975):
    H, d, n = states.shape
    (sl, su), (ol, ou) = ranks(n, interval)
    smp = r["samples"]
    if smp is not None:
        assert np.array_equal(smp[:, :d], states)
        assert np.array_equal(smp[:, d + 1], etas)
        assert np.array_equal(smp[:, d + 2], obs)
    for h in range(H):
        srt = np.sort(states[h], axis=1)
        assert np.array_equal(r["state_lower"][h], srt[:, sl]) and np.array_equal(r["state_upper"][h], srt[:, su])
        for name, a in (("eta", etas[h]), ("obs", obs[h])):
            sa = np.sort(a)
            assert r[f"{name}_lower"][h] == sa[ol] and r[f"{name}_upper"][h] == sa[ou], name
            np.testing.assert_allclose(r[f"{name}_mean"][h], np.mean(a), rtol=1e-12, atol=1e-13)
        np.testing.assert_allclose(r["state_mean"][h], states[h].mean(axis=1), rtol=1e-12, atol=1e-13)


MODELS = ["c2", "c3", "negbin", "zip", "bernoulli", "studentt", "linear", "gbsg", "euler", "beta_scaled"]


@pytest.mark.parametrize("name", MODELS)
def test_forecast_matches_the_oracle_chain_bit_for_bit(name, twin):
    model, t, y, has = case(name)
    g = NativePf(model, N, cases.SEED)
    g.run(t, y, has)
    cloud = g.particles()
    times = horizon_times(float(t[-1]))
    r = g.forecast(times, KEY, 0.975, want_samples=True)
    states, etas, obs = expected(model, cloud, float(t[-1]), times, KEY, twin)
    check_forecast(r, states, etas, obs)
    # gamma row: f(x, t) -- link(gamma) is the eta the oracle states
    d = g.d
    assert np.all(np.isfinite(r["samples"][:, d]))
    # the stateless seam draws the same observations for the same etas
    e = np.ascontiguousarray(etas[2]); out = np.zeros(N)
    desc = model.descriptor(); L = desc.leaf_array[0]
    _abi.check(g.lib.cssm_obs_draw(desc.desc.obs_kind, e.ctypes.data_as(_dp), N, L.has_scale, L.scale, desc.desc.obs_df, KEY, 2,
                                   out.ctypes.data_as(_dp), 0))
    assert np.array_equal(out, obs[2])
    g.close()


def _cloud_case(setup, twin):
    model = cases.c2_model()
    g = NativePf(model, N, cases.SEED)
    t_cloud = setup(g)
    cloud = g.particles()
    times = horizon_times(t_cloud)
    r = g.forecast(times, KEY, 0.9, want_samples=True)
    check_forecast(r, *expected(model, cloud, t_cloud, times, KEY, twin), interval=0.9)
    return g, cloud


def test_cloud_right_after_init(twin):
    def setup(g):
        g.init(0.0)
        return 0.0
    g, cloud = _cloud_case(setup, twin)
    o = oracle.OraclePf(cases.c2_model().descriptor(), N, cases.SEED); o.init(0.0)
    assert np.array_equal(cloud, o.particles())


@pytest.mark.parametrize("how", ["weighted", "unweighted", "stratified", "no_fused_sums"])
def test_cloud_after_steps(how, twin):
    t, y, has = cases.poisson_counts(3)

    def setup(g):
        if how == "stratified":
            g.set_option(2, 1)
        if how == "no_fused_sums":
            g.set_option(3, 0)
        g.init(0.0)
        g.step(1.0, 3.0)
        if how == "unweighted":
            g.step(2.0, None)
            return 2.0
        return 1.0
    g, cloud = _cloud_case(setup, twin)
    o = oracle.OraclePf(cases.c2_model().descriptor(), N, cases.SEED, flags=0)
    if how == "stratified":
        return   # (the oracle's stratified path is checked by the parity tests; here the cloud the handle holds is the source)
    o.init(0.0); o.step(1.0, 3.0)
    if how == "unweighted":
        o.step(2.0, None, False)
    assert np.array_equal(cloud, o.particles())


def test_between_propagate_and_adopt_the_proposed_cloud_is_forecast(twin):
    model = cases.c2_model()
    g = NativePf(model, N, cases.SEED)
    g.init(0.0)
    g.step(1.0, 2.0)
    g.propagate(2.0, 4.0)
    proposed = g.proposed()
    assert np.array_equal(g.particles(), proposed)
    m, lo, hi, _, _, _ = g.summary(0.975)
    times = horizon_times(2.0)
    r = g.forecast(times, KEY, 0.975, want_samples=True)
    check_forecast(r, *expected(model, proposed, 2.0, times, KEY, twin))
    np.testing.assert_allclose(m, proposed.mean(axis=1), rtol=1e-12, atol=1e-13)


def test_batch_chain_views_forecast_their_chain(twin):
    model = cases.c2_model()
    t, y, has = cases.poisson_counts(STEPS)
    b = NativePfBatch(model, N, 2)
    _, _, rc = b.filter([model, model], [11, 12], t, y, has)
    assert list(rc) == [0, 0]
    for k in range(2):
        v = b.chain(k)
        cloud = v.particles()
        times = horizon_times(float(t[-1]))
        r = v.forecast(times, KEY, 0.975, want_samples=True)
        check_forecast(r, *expected(model, cloud, float(t[-1]), times, KEY, twin))
    b.close()


def test_forecast_leaves_the_filter_untouched():
    model = cases.c2_model()
    t, y, has = cases.poisson_counts(8)
    fa = Filter(model, Resampling.systematicResampling, seed=cases.SEED)
    fb = Filter(model, Resampling.systematicResampling, seed=cases.SEED)
    sa, sb = fa.initialiseState(N, 0.0), fb.initialiseState(N, 0.0)
    for i in range(len(t)):
        before = sa
        if i in (0, 3, 5):
            ParticleFilter.forecast(sa, model, [float(t[i]) + 0.5, float(t[i]) + 2.0])
            _ = before.particles          # the PfState taken before the forecast is still current
        sa = fa.stepFilter(sa, Data(float(t[i]), float(y[i])))
        sb = fb.stepFilter(sb, Data(float(t[i]), float(y[i])))
        assert (sa.ll, sa.ess) == (sb.ll, sb.ess)
        assert np.array_equal(fa._pf.ancestors(), fb._pf.ancestors())
        assert np.array_equal(sa.particles, sb.particles)
    # the batch call continues identically too
    la = fa._pf.run_more([9.0, 10.0], [2.0, 1.0])
    lb = fb._pf.run_more([9.0, 10.0], [2.0, 1.0])
    assert la[0] == lb[0] and np.array_equal(la[2], lb[2])


def test_keys_reproduce_and_differ():
    model = cases.c2_model()
    f = Filter(model, Resampling.systematicResampling, seed=cases.SEED)
    s = f.initialiseState(N, 0.0)
    s = f.stepFilter(s, Data(1.0, 2.0))
    g = f._pf
    a = g.forecast([2.0, 3.0], KEY, want_samples=True)
    b = g.forecast([2.0, 3.0], KEY, want_samples=True)
    c = g.forecast([2.0, 3.0], KEY + 1, want_samples=True)
    assert np.array_equal(a["samples"], b["samples"])
    assert not np.array_equal(a["samples"][:, -1], c["samples"][:, -1])
    # the default key: the same state twice -> the same forecast; the next state -> another key
    k1 = g.forecast_key()
    o1 = ParticleFilter.getForecast(s, model, 2.0)
    o2 = ParticleFilter.getForecast(s, model, 2.0)
    assert np.array_equal(o1.observation, o2.observation) and np.array_equal(o1.sdeState, o2.sdeState)
    assert k1 == int(g.lib.cssm_pf_run_key(cases.SEED, (1 << 63) | 1))
    s = f.stepFilter(s, Data(2.0, 3.0))
    assert g.forecast_key() != k1


def test_chunked_forecast_equals_the_unchunked_one():
    model = cases.c3_model()   # d = 9: 11 rows per horizon
    g = NativePf(model, N, cases.SEED)
    t, y, has = cases.poisson_counts(STEPS)
    g.run(t, y, has)
    times = horizon_times(float(t[-1]))
    whole = g.forecast(times, KEY, want_samples=True)
    per_horizon_kib = (g.d + 2) * N * 8 / 1024
    for cap_kib in (int(2 * per_horizon_kib) + 1, 1):   # two horizons per chunk, then one
        g.set_option(11, cap_kib)
        part = g.forecast(times, KEY, want_samples=True)
        for k, v in whole.items():
            if isinstance(v, np.ndarray):
                assert np.array_equal(v, part[k]), k
    g.set_option(11, 0)


@pytest.mark.slow
def test_large_cloud_final_horizon_matches_the_oracle(twin):
    n = 1 << 22
    model = cases.c2_model()
    g = NativePf(model, n, cases.SEED)
    t, y, has = cases.poisson_counts(2)
    g.run(t, y, has)
    cloud = g.particles()
    times = float(t[-1]) + np.arange(1, 9, dtype=np.float64) * 0.75
    g.set_option(11, 512 * 1024)   # 512 MiB: 160 MiB of keys per horizon -> chunks of 3
    r = g.forecast(times, KEY, 0.975, want_samples=True)
    states, etas, obs = expected(model, cloud, float(t[-1]), times, KEY, twin)
    d = g.d
    assert np.array_equal(r["samples"][-1, :d], states[-1])
    assert np.array_equal(r["samples"][-1, d + 1], etas[-1])
    assert np.array_equal(r["samples"][-1, d + 2], obs[-1])
    (sl, su), (ol, ou) = ranks(n, 0.975)
    sa = np.sort(obs[-1])
    assert r["obs_lower"][-1] == sa[ol] and r["obs_upper"][-1] == sa[ou]
    np.testing.assert_allclose(r["state_mean"][-1], states[-1].mean(axis=1), rtol=1e-12, atol=1e-13)


def test_errors_name_their_cause():
    lib = _abi.load_library()

    def rc_of(g, times, interval=0.975):
        tt = np.ascontiguousarray(times, dtype=np.float64)
        return lib.cssm_pf_forecast(g._h, tt.ctypes.data_as(_dp), len(tt), KEY, interval, *([None] * 10))

    lg = NativePf(cases.c4_model(), 256, 1, lgcp_precision=2)
    lg.init(0.0)
    assert rc_of(lg, [1.0]) == _abi.CSSM_EINVAL_ARG and b"LogGaussianCox" in lib.cssm_last_error()
    g = NativePf(cases.c2_model(), 256, 1)
    assert rc_of(g, [1.0]) == _abi.CSSM_ESTATE and b"not initialised" in lib.cssm_last_error()
    g.init(2.0)
    assert rc_of(g, [1.0]) == _abi.CSSM_EINVAL_ARG and b"before the cloud's time" in lib.cssm_last_error()
    assert rc_of(g, [3.0, 2.5]) == _abi.CSSM_EINVAL_ARG and b"non-decreasing" in lib.cssm_last_error()
    for bad in (0.0, -0.1, 1.5, math.nan):
        assert rc_of(g, [3.0], bad) == _abi.CSSM_EINVAL_ARG and b"interval" in lib.cssm_last_error()
    assert rc_of(g, [3.0], 1.0) == _abi.CSSM_OK
    bt = NativePf(cases.beta_model(), 256, 1)   # Beta without a scale: the filter runs, the observation cannot be drawn
    bt.init(0.0)
    assert rc_of(bt, [1.0]) == _abi.CSSM_EINVAL_ARG and b"Must provide shape parameter for Beta Model" in lib.cssm_last_error()
    h = C.c_void_p()
    _abi.check(lib.cssm_pf_create_shard(cases.c2_model().descriptor().ptr(), 512, 0, 256, 1, 0, None, C.byref(h)))
    try:
        tt = np.array([1.0])
        rc = lib.cssm_pf_forecast(h, tt.ctypes.data_as(_dp), 1, KEY, 0.975, *([None] * 10))
        assert rc == _abi.CSSM_ESTATE and b"sharded" in lib.cssm_last_error()
    finally:
        lib.cssm_pf_destroy(h)
    f = Filter(cases.c2_model(), Resampling.systematicResampling)
    s = f.initialiseState(64, 0.0)
    with pytest.raises(ValueError):
        ParticleFilter.forecast(s, cases.c1_model(), [1.0])


def test_python_mirror():
    model = cases.c2_model()
    f = Filter(model, Resampling.systematicResampling, seed=cases.SEED)
    s = f.initialiseState(N, 0.0)
    for i, (tt, yy) in enumerate(zip(*cases.poisson_counts(3)[:2])):
        s = f.stepFilter(s, Data(float(tt), float(yy)))
    one = ParticleFilter.getMeanForecast(s, model, 4.5, 0.95)
    many = ParticleFilter.forecast(s, model, [4.5], 0.95)[0]
    assert one.t == many.t and one.obs == many.obs and one.obsIntervals == many.obsIntervals and one.eta == many.eta
    assert one.etaIntervals == many.etaIntervals and np.array_equal(one.state, many.state) and one.stateIntervals == many.stateIntervals
    outs = ParticleFilter.forecast(s, model, [4.5, 6.0, 12.0], 0.95)
    for o in outs:
        assert o.obsIntervals.lower <= o.obs <= o.obsIntervals.upper
        assert o.etaIntervals.lower <= o.eta <= o.etaIntervals.upper
        assert all(ci.lower <= m <= ci.upper for ci, m in zip(o.stateIntervals, o.state))
        back = F.forecast_out_from_csv(F.forecast_out_csv(o))
        assert (back.t, back.obs, back.obsIntervals, back.eta, back.etaIntervals) == (o.t, o.obs, o.obsIntervals, o.eta, o.etaIntervals)
        assert np.array_equal(back.state, o.state) and back.stateIntervals == o.stateIntervals
    fo = ParticleFilter.getForecast(s, model, 4.5)
    assert fo.sdeState.shape == (3, N) and fo.observation.shape == (N,)
    np.testing.assert_allclose(fo.eta, np.exp(fo.gamma), rtol=1e-15)
    # the seeded call and the default-key call of getMeanForecast agree with getForecast's draws
    assert abs(float(np.mean(fo.observation)) - one.obs) <= 1e-12 * max(1.0, abs(one.obs))
    # FilterInit: the replicated initial state forecasts like any cloud
    fi = FilterInit(model, Resampling.systematicResampling, [0.1, 0.2, -0.3])
    si = fi.initialiseState(512, 0.0)
    assert len(ParticleFilter.forecast(si, model, [1.0, 2.0])) == 2
