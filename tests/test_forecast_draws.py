"""The observation samplers of include/cssm_obs_draws.h on the host (the twin tests/cpp/obs_draw_twin.c, built with gcc the way the
numerics contract prescribes), the ForecastOut CSV line, and the forecast entry points on a host without a GPU.

Distribution checks run 2e5 draws at fixed keys: the outcome is deterministic, the thresholds (p > 1e-4) are those of a test that
would fail for a wrong sampler, not a flaky one."""
from __future__ import annotations

import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import cases
from composablestatespacemodels_amd import _abi, load_library
from composablestatespacemodels_amd import formats as F
from composablestatespacemodels_amd.filter import CredibleInterval, Filter, ForecastOut, ParticleFilter, Resampling

stats = pytest.importorskip("scipy.stats")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_dp = C.POINTER(C.c_double)
POISSON, GAUSSIAN, LGCP, NEGBIN, ZIP, BERNOULLI, STUDENT_T, BETA = 0, 1, 2, 3, 4, 5, 6, 7
N = 200_000
KEY = 0x5EED_F0CA_57


def build_twin(out_dir) -> C.CDLL:
    so = os.path.join(str(out_dir), "obs_draw_twin.so")
    subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-mfma", "-std=c99", "-shared", "-fPIC", "-o", so,
                           os.path.join(ROOT, "tests", "cpp", "obs_draw_twin.c"), "-lm"])
    lib = C.CDLL(so)
    lib.twin_obs_draw.argtypes = [C.c_int, _dp, C.c_size_t, C.c_int, C.c_double, C.c_int, C.c_uint64, C.c_uint32, _dp]
    lib.twin_obs_draw_at.argtypes = [C.c_int, C.c_double, C.c_int, C.c_double, C.c_int, C.c_uint64, C.c_uint64, C.c_uint32,
                                     C.POINTER(C.c_uint32)]
    lib.twin_obs_draw_at.restype = C.c_double
    lib.twin_gamma.argtypes = [C.c_double, C.c_size_t, C.c_uint64, C.c_uint32, _dp]
    lib.twin_poisson_from.argtypes = [C.c_double, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32]
    lib.twin_poisson_from.restype = C.c_double
    return lib


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    return build_twin(tmp_path_factory.mktemp("twin"))


def draws(twin, kind, eta, n=N, has_scale=0, scale=0.0, df=0, key=KEY, step=0):
    e = np.ascontiguousarray(np.broadcast_to(np.asarray(eta, dtype=np.float64), (n,)))
    out = np.zeros(n)
    rc = twin.twin_obs_draw(kind, e.ctypes.data_as(_dp), n, has_scale, float(scale), df, key, step, out.ctypes.data_as(_dp))
    assert rc == 0
    return out


def chi2_pvalue(x, pmf, kmax):
    """Pearson chi-square of integer draws against pmf on 0..kmax-1 plus the tail, cells merged to >= 5 expected counts."""
    k = np.arange(kmax)
    p = np.append(pmf(k), 0.0)
    p[-1] = max(0.0, 1.0 - p[:-1].sum())
    obs = np.bincount(np.minimum(x.astype(np.int64), kmax), minlength=kmax + 1)[:kmax + 1].astype(float)
    exp = p * x.size
    o2, e2, ao, ae = [], [], 0.0, 0.0
    for oi, ei in zip(obs, exp):
        ao += oi; ae += ei
        if ae >= 5.0:
            o2.append(ao); e2.append(ae); ao = ae = 0.0
    if ae > 0 and e2:
        o2[-1] += ao; e2[-1] += ae
    o2, e2 = np.array(o2), np.array(e2)
    return stats.chisquare(o2, e2 * o2.sum() / e2.sum()).pvalue


@pytest.mark.parametrize("lam", [1e-3, 0.5, 3.0, np.nextafter(10.0, 0.0), 10.0, 30.0])
def test_poisson_matches_its_distribution(twin, lam):
    x = draws(twin, POISSON, lam)
    assert np.all(x == np.floor(x)) and np.all(x >= 0)
    assert chi2_pvalue(x, stats.poisson(lam).pmf, int(lam + 8 * math.sqrt(lam) + 8)) > 1e-4


def test_poisson_at_a_large_rate(twin):
    lam = 1e4
    x = draws(twin, POISSON, lam)
    assert np.all(x == np.floor(x))
    # the exact cdf at the continuity-corrected points
    u = stats.poisson(lam).cdf(x - 0.5) + stats.poisson(lam).pmf(x) * 0.5
    assert stats.kstest(u, "uniform").pvalue > 1e-4
    assert abs(x.mean() - lam) < 5 * math.sqrt(lam / N)


@pytest.mark.parametrize("shape", [0.1, 0.5, 1.0, 2.5, 30.0])
def test_gamma_matches_its_distribution(twin, shape):
    out = np.zeros(N)
    twin.twin_gamma(shape, N, KEY, 3, out.ctypes.data_as(_dp))
    assert np.all(out >= 0)
    assert stats.kstest(out, stats.gamma(shape).cdf).pvalue > 1e-4


def test_negative_binomial(twin):
    size, mu = 3.0, 4.0
    x = draws(twin, NEGBIN, mu, has_scale=1, scale=math.log(size))
    assert chi2_pvalue(x, stats.nbinom(size, size / (size + mu)).pmf, 40) > 1e-4


@pytest.mark.parametrize("df", [1, 3, 5])
def test_students_t(twin, df):
    v, eta = 0.6, 0.5
    x = draws(twin, STUDENT_T, eta, has_scale=1, scale=math.log(v), df=df)
    assert stats.kstest((x - eta) / v, stats.t(df).cdf).pvalue > 1e-4


@pytest.mark.parametrize("a,b", [(0.3, 2.0), (4.0, 0.5)])
def test_beta_takes_the_stored_scale_as_it_is(twin, a, b):
    x = draws(twin, BETA, a, has_scale=1, scale=b)
    assert np.all((x >= 0) & (x <= 1))
    assert stats.kstest(x, stats.beta(a, b).cdf).pvalue > 1e-4


def test_zero_inflated_poisson(twin):
    v, lam = -0.8, 2.0
    p = math.exp(v) / (1 + math.exp(v))
    x = draws(twin, ZIP, lam, has_scale=1, scale=v)
    pmf = lambda k: (1 - p) * stats.poisson(lam).pmf(k) + p * (k == 0)
    assert chi2_pvalue(x, pmf, 16) > 1e-4


def test_bernoulli_and_its_clamp(twin):
    x = draws(twin, BERNOULLI, 0.3)
    assert set(np.unique(x)) == {0.0, 1.0}
    assert stats.binomtest(int(x.sum()), N, 0.3).pvalue > 1e-4
    # link clamps gamma beyond +-6 to exactly 1 and 0: the draws are then certain
    assert np.all(draws(twin, BERNOULLI, 1.0, n=5000) == 1.0)
    assert np.all(draws(twin, BERNOULLI, 0.0, n=5000) == 0.0)


def test_gaussian(twin):
    sd, eta = 0.7, -1.25
    x = draws(twin, GAUSSIAN, eta, has_scale=1, scale=math.log(sd))
    assert stats.kstest(x, stats.norm(eta, sd).cdf).pvalue > 1e-4


def test_poisson_edges(twin):
    assert np.all(draws(twin, POISSON, 0.0, n=100) == 0.0)
    assert np.all(np.isposinf(draws(twin, POISSON, math.inf, n=100)))
    assert np.all(np.isnan(draws(twin, POISSON, math.nan, n=100)))
    # beyond 2^52 the normal limit: integers, within a few sd of the rate
    big = 2.0 ** 60
    x = draws(twin, POISSON, big, n=1000)
    assert np.all(x == np.floor(x)) and np.all(np.abs(x - big) < 8 * math.sqrt(big))


def test_counter_keying(twin):
    """Key, particle, horizon and attempt each select other Philox blocks."""
    def at(kind, eta, key=KEY, gid=5, step=2, has_scale=0, scale=0.0):
        return twin.twin_obs_draw_at(kind, eta, has_scale, scale, 0, key, gid, step, None)
    base = [at(GAUSSIAN, 0.0, has_scale=1)]
    for kw in ({"key": KEY + 1}, {"gid": 6}, {"step": 3}):
        assert at(GAUSSIAN, 0.0, has_scale=1, **kw) != base[0]
    assert at(GAUSSIAN, 0.0, has_scale=1) == base[0]
    # attempts: the PTRS draw started at block 1 instead of 0 differs for some particles, and equals the draw of a stream that
    # consumed one block first
    a0 = np.array([twin.twin_poisson_from(30.0, KEY, g, 0, 0) for g in range(200)])
    a1 = np.array([twin.twin_poisson_from(30.0, KEY, g, 0, 1) for g in range(200)])
    assert np.any(a0 != a1)
    # a rejection loop consumes one block per attempt: the block count varies between particles
    used = []
    for g in range(400):
        b = C.c_uint32()
        twin.twin_obs_draw_at(POISSON, 30.0, 0, 0.0, 0, KEY, g, 0, C.byref(b))
        used.append(b.value)
    assert min(used) == 1 and max(used) > 1


def test_draws_are_reproducible_across_builds(twin, tmp_path):
    other = build_twin(tmp_path)
    for kind, eta, hs, sc, df in [(POISSON, 30.0, 0, 0.0, 0), (NEGBIN, 4.0, 1, 1.1, 0), (BETA, 0.3, 1, 2.0, 0), (STUDENT_T, 0.1, 1, 0.0, 3)]:
        a = draws(twin, kind, eta, n=2000, has_scale=hs, scale=sc, df=df)
        b = draws(other, kind, eta, n=2000, has_scale=hs, scale=sc, df=df)
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64))


def test_models_without_a_scale_or_an_observation_are_refused(twin):
    e = np.ones(4); out = np.zeros(4)
    for kind in (GAUSSIAN, NEGBIN, ZIP, STUDENT_T, BETA):
        assert twin.twin_obs_draw(kind, e.ctypes.data_as(_dp), 4, 0, 0.0, 3, KEY, 0, out.ctypes.data_as(_dp)) == -1
    assert twin.twin_obs_draw(LGCP, e.ctypes.data_as(_dp), 4, 0, 0.0, 0, KEY, 0, out.ctypes.data_as(_dp)) == -2


def test_forecast_out_csv_prints_the_case_class_to_string():
    o = ForecastOut(3.5, 2.25, CredibleInterval(0.0, 7.0), 2.125, CredibleInterval(0.5, 6.5), np.array([0.1, -0.2]),
                    [CredibleInterval(-1.0, 1.0), CredibleInterval(-2.0, 2.5)])
    line = F.forecast_out_csv(o)
    assert line == ("3.5, 2.25, CredibleInterval(0.0,7.0), 2.125, CredibleInterval(0.5,6.5), 0.1, -0.2, "
                    "CredibleInterval(-1.0,1.0), CredibleInterval(-2.0,2.5)")
    back = F.forecast_out_from_csv(line)
    assert (back.t, back.obs, back.obsIntervals, back.eta, back.etaIntervals) == (o.t, o.obs, o.obsIntervals, o.eta, o.etaIntervals)
    assert np.array_equal(back.state, o.state) and back.stateIntervals == o.stateIntervals


def test_forecast_symbols_are_declared_and_bound():
    lib = load_library()
    bound = {s[0] for s in _abi.SYMBOLS}
    for name in ("cssm_pf_forecast", "cssm_pf_forecast_last_ms", "cssm_pf_observation_index", "cssm_obs_draw"):
        assert hasattr(lib, name) and name in bound
    assert lib.cssm_pf_forecast(None, None, 0, 0, 0.975, *([None] * 10)) == _abi.CSSM_EINVAL_ARG


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="this check is for hosts without a GPU")
def test_forecasts_fail_loudly_without_gpu():
    lib = load_library()
    e = np.ones(8); out = np.zeros(8)
    rc = lib.cssm_obs_draw(POISSON, e.ctypes.data_as(_dp), 8, 0, 0.0, 0, KEY, 0, out.ctypes.data_as(_dp), 0)
    assert rc == _abi.CSSM_EHIP
    assert b"no CPU path" in lib.cssm_last_error()
    with pytest.raises(_abi.CssmError) as ei:
        f = Filter(cases.c2_model(), Resampling.systematicResampling)
        s = f.initialiseState(64, 0.0)
        ParticleFilter.forecast(s, cases.c2_model(), [1.0, 2.0])
    assert ei.value.code == _abi.CSSM_EHIP
