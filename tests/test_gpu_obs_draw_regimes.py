"""-m gpu: the observation samplers of include/cssm_obs_draws.h on the real kernels with the lanes of one wavefront in DIFFERENT regimes.

The forecasts and simulations of the test models reach moderate etas only, and neighbouring lanes fall into the same branch of every
sampler.  Here every lane gets a state -- and, through cssm_pf_forecast_posterior, a scale -- of its own, taken from a table with an entry
per regime and per regime edge and interleaved so that lane i and lane i + 1 never share a regime: Poisson's early returns (eta = 0,
+inf), inversion, PTRS with either form of its exponent and the normal limit; Gamma with and without the boost of shape < 1; the clamps
of Bernoulli's link.  That is where a data-dependent loop with a per-lane block counter goes wrong on a GPU and nowhere else.

Two entry points take per-lane states: cssm_simulate_from (times = [t0, t0]: dt = 0 leaves a Brownian state where it is, and each time
index draws under a step of its own) and cssm_pf_forecast_posterior / cssm_fleet_forecast_posterior (a pair (theta, x) per particle,
pick = the identity).  Expected values: eta from the oracle's link (and, for the log links, oracle.c_exp) and the observation from the
host twin's twin_obs_draw_at per (kind, eta, scale, df, key, particle, step); both rows compared bit for bit, NaN placement included.

No law is tested here: tests/test_obs_draw_laws.py holds the twin to the law of every sampler over its whole range, this file and the
forecast / simulate tests hold the device to the twin -- here also where lanes diverge.  Before comparing, each case asserts on the host
that its table really puts >= 3 regimes into every wavefront and (for the samplers that have a rejection loop) that the twin's block
counts differ within it."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import pytest

from composablestatespacemodels_amd import CssmError, _abi
from composablestatespacemodels_amd.filter import NativePf, NativePfFleet
from composablestatespacemodels_amd.model import Model, Parameters, Sde, SdeParameter
from composablestatespacemodels_amd.simulate import simulate_from
from oracle import oracle
from test_forecast_draws import BERNOULLI, BETA, NEGBIN, POISSON, STUDENT_T, ZIP, build_twin
from test_gpu_forecast_posterior import params_of

pytestmark = pytest.mark.gpu

KEY = 0x0B5D_4A3E
SIZES = [1, 63, 64, 65, 2 * 256 + 1]      # a wave absent, ragged, full, full + 1 lane, and more than one block
WAVE = 64
T0, FIRST_STEP = 1.5, 5
CUT, NORMAL_MIN = 2.0 ** 26, 2.0 ** 52    # CSSM_OBS_PTRS_DELTA_MIN, CSSM_OBS_NORMAL_MIN
SCALES = [0.05, float(np.nextafter(1.0, 0.0)), 1.0, 3.0, 1e6]     # NegBin size / Beta b per particle: the boost of shape < 1 and its absence


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    return build_twin(tmp_path_factory.mktemp("twin"))


def brownian(obs, leaves=1, scale=None, df=None):
    """`leaves` one-dimensional Brownian leaves (gamma = the sum of the components) under observation model `obs`."""
    make = {"poisson": Model.poisson, "zip": Model.zeroInflatedPoisson, "bernoulli": Model.bernoulli, "negbin": Model.negativeBinomial,
            "beta": Model.beta}.get(obs)
    sde = Sde.brownianMotion(1)
    um = Model.studentsT(sde, df) if obs == "studentt" else make(sde)
    ps = Parameters.apply(scale, SdeParameter.brownianParameter(0.0, 1.0, 0.3))
    for _ in range(leaves - 1):
        um = um | Model.poisson(sde)
        ps = ps | Parameters.apply(None, SdeParameter.brownianParameter(0.0, 1.0, 0.3))
    return um.run(ps)


def straddle(threshold, lo, hi):
    """The adjacent doubles (x, x+) with cssm_exp(x) < threshold <= cssm_exp(x+)  (threshold = inf: the last finite one and the first +inf)."""
    ge = lambda x: bool(oracle.c_exp(np.array([x]))[0] >= threshold)
    assert not ge(lo) and ge(hi)
    while float(np.nextafter(lo, hi)) != hi:
        mid = 0.5 * (lo + hi)
        lo, hi = (lo, mid) if ge(mid) else (mid, hi)
    return lo, hi


def log_link_gammas():
    at10, at_cut, at_normal, at_inf = straddle(10.0, 2.0, 3.0), straddle(CUT, 18.0, 19.0), straddle(NORMAL_MIN, 36.0, 37.0), straddle(math.inf, 709.0, 710.0)
    return [-745.5, -709.0, float(np.nextafter(-708.0, -1e9)),            # eta = 0
            -708.0, -700.0, -3.0, 0.0, 1.0, at10[0],                       # inversion
            at10[1], 3.4, 9.2, 13.8, at_cut[0],                            # PTRS, the exponent as written
            at_cut[1], 20.0, 27.6, 34.5, at_normal[0],                     # PTRS, the exponent from k - lambda
            at_normal[1], 41.4, 300.0, 709.0, at_inf[0],                   # the normal limit
            at_inf[1], 720.0, 1e6]                                         # +inf


def poisson_regime(eta):
    if eta != eta: return "nan"
    if eta == 0.0: return "zero"
    if eta == math.inf: return "inf"
    if eta < 10.0: return "inversion"
    if eta < CUT: return "ptrs"
    if eta < NORMAL_MIN: return "ptrs-delta"
    return "normal"


def bernoulli_regime(eta):
    return "zero" if eta == 0.0 else ("one" if eta == 1.0 else "interior")


def gamma_regime(eta):
    if not (eta > 0.0) or eta == math.inf: return "early"
    return "boost" if eta < 1.0 else "plain"


BERNOULLI_GAMMAS = [-1e300, -7.0, float(np.nextafter(-6.0, -7.0)), -6.0, -2.0, 0.0, 2.0, 6.0, float(np.nextafter(6.0, 7.0)), 7.0, 1e300]
# (Beta's link is the log link: eta = exp(gamma) is its first shape)
BETA_GAMMAS = [-745.5, -709.0, 720.0, 1e6, -700.0, -6.9, -1.2, float(np.nextafter(0.0, -1.0)), -1.2e-16, 0.0, 1.2e-16, 1.4, 6.9, 13.8, 700.0]


def link_of(model, d, gammas):
    """eta of the states (g, 0, ..): the oracle's link, one state at a time"""
    o = oracle.OraclePf(model.descriptor(), 1, KEY)
    o.init(T0)
    return np.array([o.eta_of(np.array([g] + [0.0] * (d - 1))) for g in gammas])


def interleave(gammas, etas, regime):
    """The table reordered so that consecutive entries (cyclically) never share a regime: a round robin over the regimes, each cycling
    through its own entries."""
    groups = {}
    for g, e in zip(gammas, etas):
        groups.setdefault(regime(float(e)), []).append(g)
    names = sorted(groups)
    assert len(names) >= 3, names
    longest = max(len(v) for v in groups.values())
    return [groups[r][j % len(groups[r])] for j in range(longest) for r in names]


def lanes(table, n):
    return np.array([table[i % len(table)] for i in range(n)])


def assert_mixed(etas, regime, blocks=None):
    """every wavefront holds >= 3 regimes (as many as it has lanes, below three), no two neighbours share one, and the twin's block counts
    differ within it"""
    r = [regime(float(e)) for e in etas]
    assert all(a != b for a, b in zip(r, r[1:]))
    for w in range(0, len(r), WAVE):
        assert len(set(r[w:w + WAVE])) >= min(3, len(r[w:w + WAVE])), (w, set(r[w:w + WAVE]))
        if blocks is not None and len(r[w:w + WAVE]) >= 8:
            assert len(set(blocks[w:w + WAVE].tolist())) > 1, w


def twin_rows(twin, kind, etas, scales, df, key, steps):
    """(obs[H, n], blocks[H, n]) of the twin: particle i under eta[i], scale[i] at every step"""
    n = len(etas)
    obs, blocks = np.zeros((len(steps), n)), np.zeros((len(steps), n), dtype=np.int64)
    for h, step in enumerate(steps):
        for i in range(n):
            b = C.c_uint32()
            has = 0 if scales is None else 1
            obs[h, i] = twin.twin_obs_draw_at(kind, float(etas[i]), has, 0.0 if scales is None else float(scales[i]), df, key, i, step, C.byref(b))
            blocks[h, i] = b.value
    return obs, blocks


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64)) or (
        np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.where(np.isnan(a), 0.0, a).view(np.uint64), np.where(np.isnan(b), 0.0, b).view(np.uint64)))


# ---------------------------------------------------------------- cssm_simulate_from: Poisson, ZIP, Bernoulli

SIM_CASES = {"poisson": (POISSON, None, poisson_regime, True), "zip": (ZIP, -0.8, poisson_regime, True),
             "bernoulli": (BERNOULLI, None, bernoulli_regime, False)}


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("d", [1, 3])
@pytest.mark.parametrize("name", list(SIM_CASES))
def test_simulate_from_with_a_regime_per_lane(name, d, n, twin):
    kind, scale, regime, has_loop = SIM_CASES[name]
    model = brownian(name, leaves=d, scale=scale)
    gammas = BERNOULLI_GAMMAS if name == "bernoulli" else log_link_gammas()
    table = interleave(gammas, link_of(model, d, gammas), regime)
    g = lanes(table, n)
    eta = link_of(model, d, g)
    if name != "bernoulli":
        assert np.array_equal(eta, oracle.c_exp(g))
    steps = [FIRST_STEP, FIRST_STEP + 1]
    want, blocks = twin_rows(twin, kind, eta, None if scale is None else [scale] * n, 0, KEY, steps)
    if n >= 3:
        assert_mixed(eta, regime, blocks[0] if has_loop else None)
    x = np.zeros((d, n)); x[0] = g
    got = simulate_from(model, x, FIRST_STEP, T0, [T0, T0], KEY)
    assert got.shape == (2, d + 3, n)
    for h in range(2):
        assert np.array_equal(got[h, :d], x), "dt = 0 leaves the states where they are"
        assert np.array_equal(got[h, d], g), "gamma"
        assert same_bits(got[h, d + 1], eta), "eta"
        assert same_bits(got[h, d + 2], want[h]), ("obs", h, np.flatnonzero(got[h, d + 2] != want[h])[:8])
    if n > 1 and name != "bernoulli":
        assert np.isposinf(got[0, d + 2]).any() and (got[0, d + 2] == 0.0).any()


def test_non_finite_states_are_refused():
    model = brownian("poisson")
    for bad in (math.inf, -math.inf, math.nan):
        x = np.zeros((1, 5)); x[0, 3] = bad
        with pytest.raises(CssmError) as ei:
            simulate_from(model, x, FIRST_STEP, T0, [T0, T0], KEY)
        assert ei.value.code == _abi.CSSM_EINVAL_ARG
        with NativePf(model, 5, 1) as pf:
            theta = np.tile(np.asarray(params_of(model).flattenParams()), (5, 1))
            with pytest.raises(CssmError) as ei:
                pf.forecast_posterior(theta, x.T, T0, [T0, T0], KEY, pick=np.arange(5), want_samples=True)
            assert ei.value.code == _abi.CSSM_EINVAL_ARG


# ---------------------------------------------------------------- cssm_pf_forecast_posterior: NegBin, Beta, Student-t

def posterior_case(name, n):
    """(model, kind, df, regime, gamma[n], stored scale[n])"""
    if name == "negbin":
        model, kind, df, regime, gammas = brownian("negbin", scale=0.0), NEGBIN, 0, poisson_regime, log_link_gammas()
        stored = [math.log(0.05), -1.2e-16, 0.0, math.log(3.0), math.log(1e6)]      # size = cssm_exp(stored)
        sizes = oracle.c_exp(np.array(stored))
        assert sizes[1] == SCALES[1] and sizes[2] == 1.0 and sizes[0] < 1.0 < sizes[3] < sizes[4]
    elif name == "beta":
        model, kind, df, regime, gammas, stored = brownian("beta", scale=0.8), BETA, 0, gamma_regime, BETA_GAMMAS, SCALES      # b = the stored scale as it is
    else:
        df = int(name[1:])
        model, kind, regime, gammas, stored = brownian("studentt", scale=0.0, df=df), STUDENT_T, None, [-1e8, -1.0, 0.0, 1.0, 1e8], [-20.0, 0.0, 3.0]
    table = gammas if regime is None else interleave(gammas, link_of(model, 1, gammas), regime)
    return model, kind, df, regime, lanes(table, n), lanes(stored, n)


def posterior_rows_of(model, scales):
    theta = np.tile(np.asarray(params_of(model).flattenParams()), (len(scales), 1))
    theta[:, 0] = scales          # the flatten order of a leaf starts with its scale
    return theta


def check_posterior(r, model, kind, df, regime, g, scales, key, twin, n):
    eta = link_of(model, 1, g)
    want, blocks = twin_rows(twin, kind, eta, scales, df, key, [0, 1])
    if regime is not None and n >= 3:
        assert_mixed(eta, regime)
    if regime is None:      # Student-t: one regime per call (df belongs to the model); its lanes differ in their attempts alone
        # (at shape 1.5 the acceptance is ~0.98, 64 lanes may all take the first attempt; at shape 500 it is so close to 1 that all 1026
        # draws do: that row runs the kernel's per-lane scales, its lanes do not diverge)
        assert n < SIZES[-1] or df != 1 or len(set(blocks.ravel().tolist())) > 1
    else:
        for w in range(0, n, WAVE):
            if n - w >= 8:
                assert len(set(blocks[0, w:w + WAVE].tolist())) > 1, w
    smp = r["samples"]
    assert smp.shape == (2, 4, n) and np.array_equal(r["pick"], np.arange(n))
    for h in range(2):
        assert np.array_equal(smp[h, 0], g) and np.array_equal(smp[h, 1], g), "state and gamma"
        assert same_bits(smp[h, 2], eta), "eta"
        assert same_bits(smp[h, 3], want[h]), ("obs", h, np.flatnonzero(~((smp[h, 3] == want[h]) | (np.isnan(smp[h, 3]) & np.isnan(want[h]))))[:8])
    return want


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", ["negbin", "beta", "t1", "t1000"])
def test_forecast_posterior_with_a_regime_and_a_scale_per_lane(name, n, twin):
    model, kind, df, regime, g, scales = posterior_case(name, n)
    with NativePf(model, n, 1) as pf:
        r = pf.forecast_posterior(posterior_rows_of(model, scales), g[:, None], T0, [T0, T0], KEY, pick=np.arange(n), want_samples=True)
    want = check_posterior(r, model, kind, df, regime, g, scales, KEY, twin, n)
    if name == "beta" and n >= 64:
        assert np.isnan(want).any() and not np.isnan(want).all()       # the NaN of a zero or infinite shape sits between finite lanes


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", ["negbin", "beta"])
def test_fleet_forecast_posterior_with_a_regime_and_a_scale_per_lane(name, n, twin):
    S = 3
    model, kind, df, regime, g, scales = posterior_case(name, n)
    keys = [KEY + 17 * k for k in range(S)]
    # series k starts the cycle of scales elsewhere: other (regime, scale) pairs on the same lanes, and a key of its own
    gs, ss = [g] * S, [np.roll(scales, k) if n >= len(SCALES) else scales for k in range(S)]
    post = [(posterior_rows_of(model, ss[k]), gs[k][:, None]) for k in range(S)]
    with NativePfFleet(model, n, S) as fl:
        rs = fl.forecast_posterior(post, T0, [[T0, T0]] * S, keys, 0.975, picks=np.tile(np.arange(n), (S, 1)), want_samples=True)
    for k in range(S):
        assert rs[k]["rc"] == 0
        check_posterior(rs[k], model, kind, df, regime, gs[k], ss[k], keys[k], twin, n)
