"""The grid filter (tests/grid_reference.py) as a truth that shares neither code nor variates with the kernels or the oracle.

* the grid against closed form: a d-dimensional Kalman filter for the Gaussian-observation models, 1-D and d = 3 (seasonal H(t),
  GenBrownian and OU transitions) -- the grid machinery is proven before it judges anything;
* the grid's own refinement bound and edge loss for every family the particle filters are held against (here and in
  tests/test_gpu_grid_reference.py);
* the CPU oracle, in contract mode and in LITERAL_SUMS | LIBM mode, against the grid: this pins the restatement itself.
"""
import math

import numpy as np
import pytest

import cases
import grid_reference as gr
from composablestatespacemodels_amd import Model, Parameters, Sde, SdeParameter
from composablestatespacemodels_amd.model import UnparamModel
from oracle import oracle


def c1_ou_model():
    """C1 with its Brownian motion replaced by an OU process."""
    return Model.poisson(Sde.ouProcess(1)).run(Parameters.apply(None, SdeParameter.ouParameter(0.0, 1.0, 0.2, 0.5, 0.3)))


def c1_gen_model():
    """C1 with its Brownian motion replaced by a generalised Brownian motion (drift 0.01)."""
    return Model.poisson(Sde.genBrownianMotion(1)).run(Parameters.apply(None, SdeParameter.genBrownianParameter(0.0, 1.0, 0.01, 0.02)))


def outlier_series(T=40, where=10):
    """gaussian_series with y = 60 at one step, for the Student-t model: every log-weight falls 37 below the observation's
    reference level (more than CSSM_REF_ABOVE = 32), so the kernels redo that observation's sums relative to the max.
    (A Poisson outlier that rules out the level, as test_gpu_parity._outlier_series's y = 60 under C2, puts the posterior
    8 sd into the tail of the prediction: no filter of 2^20 particles estimates that likelihood -- the replicate sd of ll
    is 4.5 there.  The heavy-tailed model discounts the outlier, so the likelihood stays estimable.)"""
    t, y, has = cases.gaussian_series(T)
    y = y.copy()
    y[where] = 60.0
    return t, y, has


def perturbed(model, index, amount):
    """The model with `amount` added to its flattened parameter `index` (Parameters.add)."""
    p = model.parameters()
    delta = [0.0] * p.paramSize()
    delta[index] = amount
    return UnparamModel([leaf[0] for leaf in model.leaves]).run(p.add(delta))


# name: (model, series, LGCP precision, (flat parameter index, amount, what it is) of the power check)
CASES = {
    "c1": (cases.c1_model, lambda: cases.poisson_counts(40), 0, (2, math.log(1.5), "sigma x 1.5")),
    "c1_ou": (c1_ou_model, lambda: cases.poisson_counts(40), 0, (4, 0.1, "sigma x 1.105")),
    "c1_gen": (c1_gen_model, lambda: cases.poisson_counts(40), 0, (2, 0.02, "mu + 0.02")),
    "euler": (cases.euler_model, lambda: cases.poisson_counts(40), 0, (7, 0.1, "g[0] + 0.1")),
    "linear": (cases.linear_model, lambda: cases.gaussian_series(40), 0, (0, 0.25, "log obs sd + 0.25")),
    "negbin": (cases.negbin_model, lambda: cases.poisson_counts(25), 0, (0, -0.5, "log size - 0.5")),
    "zip": (cases.zip_model, lambda: cases.counts_with_zeros(40), 0, (0, 0.2, "logit zero-probability + 0.2")),
    "bernoulli": (cases.bernoulli_model, lambda: cases.binary_series(40), 0, (3, 0.15, "mu + 0.15")),
    "studentt": (cases.studentt_model, lambda: cases.gaussian_series(40), 0, (0, 0.05, "log scale + 0.05")),
    "beta": (cases.beta_model, lambda: cases.unit_interval_series(40), 0, (3, 0.05, "mu + 0.05")),
    "c2": (cases.c2_model, lambda: cases.poisson_counts(20, missing=0.15), 0, (4, 0.1, "sigma[0] x 1.105")),
    "studentt_outlier": (cases.studentt_model, outlier_series, 0, (0, 0.05, "log scale + 0.05")),
    "c4": (cases.c4_model, lambda: cases.event_times(12, horizon=2.0), 2, (3, 0.1, "mu + 0.1")),
    "lgcp_seasonal": (cases.lgcp_seasonal_model, lambda: cases.event_times(8, horizon=2.0), 1, (3, 0.1, "mu[0] + 0.1")),
}
# sub-steps of 0.1 (sd 0.06) from a prior of sd 0.55 at d = 3: the default budget leaves h / sd = 1.6 and 4e-3 of error in ll
BUDGET = {"lgcp_seasonal": 2_000_000}

# The smallest Monte-Carlo tolerance any particle filter run is held to against these grids (|mean ll - grid| at N <= 2^24, R = 8:
# 4.5 s / sqrt(8) with s >= 2e-3).  The grid's own error must be a tenth of it.
MC_TOL_FLOOR = 3e-3


def case(name):
    mk, series, prec, _ = CASES[name]
    model = mk()
    t, y, has = series()
    return model, t, y, has, prec


def grid_of(name, model=None):
    m, t, y, has, prec = case(name)
    return gr.reference(model or m, t, y, has, prec, BUDGET.get(name, gr.POINT_BUDGET))


def kalman_ll(t, y, m0, c0, sigma, obs_sd):
    from test_oracle_pins import kalman_ll as k
    return k(t, y, m0, c0, sigma, obs_sd)


# --------------------------------------------------------------------------------------------- grid against closed form
@pytest.mark.parametrize("name", ["linear", "gbsg"])
def test_grid_matches_kalman(name):
    if name == "linear":
        model = cases.linear_model()
    else:
        model = cases.gen_brownian_seasonal_gaussian()
    t, y, has = cases.gaussian_series(40)
    has = has.copy()
    has[[7, 8, 21]] = 0                                   # missing observations: a prediction without a potential
    spec = gr.spec_of(model)
    kl, km, kv = gr.kalman(spec, t, y, has)
    g = gr.reference(model, t, y, has)
    print(f"\n{name}: d = {spec.d}  ll grid {g.ll:.12f}  kalman {kl[-1]:.12f}  |dll| {np.abs(g.ll_t - kl).max():.2e}  "
          f"|dmean| {np.abs(g.mean - km).max():.2e}  points {g.points}")
    np.testing.assert_allclose(g.ll_t, kl, rtol=0, atol=1e-8)
    np.testing.assert_allclose(g.mean, km, rtol=0, atol=1e-8)
    # the quantiles of a Gaussian filtering distribution, within the grid's own quantile bound
    from scipy.special import ndtri
    for q, got, err in ((0.025, g.lo, g.lo_err), (0.975, g.hi, g.hi_err)):
        assert np.all(np.abs(got - (km + ndtri(q) * np.sqrt(kv))) <= err)


def test_one_dimensional_kalman_reproduces_the_pinned_kalman():
    sigma, obs_sd, m0, c0 = 0.3, 0.5, 0.5, 2.0
    t, y, has = cases.gaussian_series(40, sigma=sigma, obs_sd=obs_sd)
    kl = gr.kalman(gr.spec_of(cases.linear_model(sigma, obs_sd, m0, c0)), t, y, has)[0]
    assert abs(kl[-1] - kalman_ll(t, y, m0, c0, sigma, obs_sd)) <= 1e-12


def test_potentials_match_scipy_stats():
    """The grid's potentials are its own; the scipy.stats distributions are a third statement of the same densities."""
    from scipy import stats
    g = np.linspace(-5.0, 5.0, 41)
    lp = lambda obs, scale, df, y: gr.log_potential(obs, scale, df, g, y)
    np.testing.assert_allclose(lp("poisson", 0, 0, 3.7), stats.poisson.logpmf(3, np.exp(g)), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(lp("linear", math.log(0.5), 0, 0.3), stats.norm.logpdf(0.3, g, 0.5), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(lp("studentt", math.log(0.6), 5, 0.3), stats.t.logpdf((0.3 - g) / 0.6, 5) / 0.6, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(lp("negbin", math.log(3.0), 0, 4.0), stats.nbinom.logpmf(4, 3.0, 3.0 / (3.0 + np.exp(g))), rtol=1e-10, atol=1e-10)
    p = 1 / (1 + math.exp(0.8))
    np.testing.assert_allclose(lp("zip", -0.8, 0, 0.0), np.log(p + (1 - p) * np.exp(-np.exp(g))), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(lp("zip", -0.8, 0, 2.0), np.log(1 - p) + stats.poisson.logpmf(2, np.exp(g)), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(lp("beta", 0, 0, 0.3), stats.beta.logpdf(0.3, np.exp(-g), 1.0), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(lp("bernoulli", 0, 0, 1.0), stats.bernoulli.logpmf(1, 1 / (1 + np.exp(-g))), rtol=1e-12)
    np.testing.assert_allclose(lp("bernoulli", 0, 0, 0.0), stats.bernoulli.logpmf(0, 1 / (1 + np.exp(-g))), rtol=1e-12)
    assert gr.log_potential("bernoulli", 0, 0, np.array([6.5, -6.5]), 0.0)[0] == -1e99
    assert gr.log_potential("bernoulli", 0, 0, np.array([6.5, -6.5]), 1.0)[1] == -1e99


# --------------------------------------------------------------------------------------------- grid refinement
@pytest.mark.parametrize("name", list(CASES))
def test_grid_is_refined_enough(name):
    g = grid_of(name)
    d = g.mean.shape[1]
    print(f"\n{name}: d = {d}  ll {g.ll:.10f}  ll_err {g.ll_err.max():.2e}  mean_err {g.mean_err.max():.2e}  lost {g.lost:.1e}  "
          f"points {g.points}  h/sd {g.h_over_sd:.2f}")
    assert g.ll_err.max() <= MC_TOL_FLOOR / 10
    assert g.mean_err.max() <= 1e-4 and g.lo_err.max() <= 1e-3 and g.hi_err.max() <= 1e-3
    assert g.lost <= 1e-12


# --------------------------------------------------------------------------------------------- the oracle against the truth
ORACLE_N, ORACLE_R = 1 << 16, 16


@pytest.mark.parametrize("name,flags", [("c1", 0), ("c2", 0), ("c2", oracle.LITERAL_SUMS | oracle.LIBM)])
def test_oracle_likelihood_converges_to_the_grid(name, flags):
    """The one-thread restatement at N = 2^16 with 16 seeds: |mean ll - grid| <= 4.5 s / sqrt(R) + 3 grid_err + s^2 / 2."""
    model, t, y, has, prec = case(name)
    T = 20
    t, y, has = t[:T], y[:T], has[:T]
    g = gr.reference(model, t, y, has, prec)
    o = oracle.OraclePf(model.descriptor(prec), ORACLE_N, 1, flags)
    lls = []
    for r in range(ORACLE_R):
        o.reseed(7000 + r)
        lls.append(o.filter(t, y, has)[0])
    lls = np.array(lls)
    s = float(lls.std(ddof=1))
    margin = 4.5 * s / math.sqrt(ORACLE_R) + 3 * float(g.ll_err[-1]) + s * s / 2
    dev = float(lls.mean() - g.ll)
    print(f"\n{'case':8} {'flags':>5} {'N':>7} {'R':>3} {'mean ll':>14} {'grid ll':>14} {'grid_err':>9} {'s':>9} {'margin':>9} {'dev':>9}\n"
          f"{name:8} {flags:5d} {ORACLE_N:7d} {ORACLE_R:3d} {lls.mean():14.8f} {g.ll:14.8f} {g.ll_err[-1]:9.2e} {s:9.2e} {margin:9.2e} {dev:+9.2e}")
    assert abs(dev) <= margin
