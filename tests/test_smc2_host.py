"""SMC2 (composablestatespacemodels_amd/smc2.py, EXTENSION) on the CPU: the driver over an ``OracleEngine`` -- S ``oracle.OraclePf``
handles running, S proposing -- which has the filter bits of the fleets, so tests/test_gpu_smc2.py holds the GPU run to it bit for bit.

What the oracle's ``adopt`` lacks for a continued step: it keeps the handle's own clock and observation index.  In lockstep every series
shares both, so adoption needs neither -- except for a DEAD handle: a failed ``oracle_pf_step`` advances neither, and the fleet's masked
series is given both by the copy.  The engine therefore keeps a dead handle in lockstep with unweighted steps (its cloud is replaced at
the next resampling; nothing reads it before).  ``oracle/`` is unchanged.

Truth.  ``cases.linear_model()`` on ``cases.gaussian_series(T)``, T = 24; free: the observation scale (log sd) and log sigma, each with a
normal prior on the unconstrained scale; ``prior_draws`` sampled from it with a fixed seed per replicate.  The exact posterior moments
and evidence: a 2-D trapezoid rule of ``grid_reference.kalman`` log-likelihoods times the prior at two spacings (h and 2 h on nested
grids); ``err`` is their difference.  R replicates of S = 128 parameter particles x N = 64 state particles, seeds SEED0 + r.  Held to
the project's criteria (tests/test_grid_smoother.py: zscore, accepted): z = (replicate mean - truth) / sqrt(s^2 / R + (3 err)^2), rms
<= 3 and max <= 8 over the posterior mean and sd of either free component and the final log evidence.

Measured here (CPU oracle, the seeds below; z per statistic in the order mean[scale], mean[log sigma], sd[scale], sd[log sigma],
log evidence; the test prints them on every run): R = 8: z = [-0.26, -0.18, -0.01, -0.20, -0.28] (accepted); the prior's moments
offered as the truth: z = [-25.0, 7.3, -14.7, -12.2] (rejected); the evidence of a run that never reweights -- sum_t log mean_k
exp(inc_t,k) of the increments of a run without rejuvenation -- z = -18.1 (rejected).  Two rejuvenations per replicate.  How R was
chosen: 16 replicates were run once and the criteria evaluated on the first 4, 8, 12 and 16 of them; all four accept the run (max |z|
0.68, 0.28, 1.49, 1.09) and reject both power checks (never-reweighted z = -11.1, -18.1, -22.1, -29.1), so R = 8 is the second
smallest: a margin over the smallest that works, at 1.5 s.  No seed was retried or dropped.  The quadrature's own error (two nested
spacings) is below 1e-6 on every statistic, three orders below the replicate scatter / sqrt(R).
"""
import numpy as np
import pytest

import cases
import grid_reference as gr
from composablestatespacemodels_amd import SMC2, Smc2State, TimedObservation, _abi
from composablestatespacemodels_amd.smc2 import logsumexp, systematic_ancestors
from oracle import oracle
from test_grid_smoother import accepted, zscore


class OracleEngine:
    """The engine protocol of smc2.FleetEngine over CPU oracle handles (one per series and side)."""

    def __init__(self, model, n, series):
        self.S, self.n = int(series), int(n)
        self.descA = [model.descriptor() for _ in range(self.S)]
        self.descB = list(self.descA)
        self.A = [oracle.OraclePf(self.descA[k], self.n, 0) for k in range(self.S)]
        self.B = [oracle.OraclePf(self.descB[k], self.n, 0) for k in range(self.S)]
        self.llA, self.essA = np.zeros(self.S), np.full(self.S, self.n, dtype=np.int64)
        self.llB, self.essB = np.zeros(self.S), np.full(self.S, self.n, dtype=np.int64)
        self.clones = self.adoptions = 0

    def init(self, models, keys, t0):
        for k, o in enumerate(self.A):
            self.descA[k] = models[k].descriptor()
            o.set_params(self.descA[k]); o.reseed(int(keys[k])); o.init(float(t0))
        self.llA[:] = 0.0; self.essA[:] = self.n

    def step(self, t, y, has, active):
        ll, rc = np.full(self.S, np.nan), np.zeros(self.S, dtype=np.int32)
        for k, o in enumerate(self.A):
            if active is not None and not active[k]:
                o.step(t, None, False)                       # (a masked handle stays in lockstep; see the module docstring)
                continue
            try:
                self.llA[k], self.essA[k] = o.step(t, y, bool(has))
                ll[k] = self.llA[k]
            except oracle.OracleError as e:
                assert e.code == oracle.ENONFINITE
                rc[k] = _abi.CSSM_ENONFINITE
                o.step(t, None, False)
        return ll, rc

    def clone(self, anc):
        snap = [(o.particles(), self.llA[k], self.essA[k], self.descA[k]) for k, o in enumerate(self.A)]
        for k, o in enumerate(self.A):
            j = int(anc[k])
            if j != k:
                x, self.llA[k], self.essA[k], self.descA[k] = snap[j]
                o.adopt(x, self.llA[k], self.essA[k]); o.set_params(self.descA[k])
        self.clones += 1

    def propose(self, models, keys, data):
        t, y, has = data
        ll, ok = np.full(self.S, np.nan), np.zeros(self.S, dtype=bool)
        for k, o in enumerate(self.B):
            self.descB[k] = models[k].descriptor()
            o.set_params(self.descB[k]); o.reseed(int(keys[k]))
            try:
                ll[k], _, ess_t, _ = o.filter(t, y, has)
                self.llB[k], self.essB[k], ok[k] = ll[k], ess_t[-1], True
            except oracle.OracleError as e:
                assert e.code == oracle.ENONFINITE
        return ll, ok

    def adopt(self, accepted):
        for k in np.flatnonzero(accepted):
            self.llA[k], self.essA[k], self.descA[k] = self.llB[k], self.essB[k], self.descB[k]
            self.A[k].adopt(self.B[k].particles(), self.llA[k], self.essA[k]); self.A[k].set_params(self.descA[k])
            self.adoptions += 1

    def reseed(self, keys):
        for k, o in enumerate(self.A):
            o.reseed(int(keys[k]))

    def summary(self, interval=0.975):
        return [o.summary(interval) for o in self.A]

    def close(self):
        self.A, self.B = [], []


# ------------------------------------------------------------------------------------------------ the truth case
T = 24
S, N = 128, 64
R = 8
SEED0 = 20260301
FREE = (0, 3)                                   # flattenParams of the linear model: [log obs sd, m0, log c0, log sigma]
PRIOR_MEAN = np.array([np.log(0.8), np.log(0.15)])
PRIOR_SD = np.array([0.5, 0.5])


def unparam():
    from composablestatespacemodels_amd import Model, Sde
    return Model.linear(Sde.brownianMotion(1))


def base_params():
    return cases.linear_model().parameters()


def log_prior(theta):
    z = (np.asarray(theta)[list(FREE)] - PRIOR_MEAN) / PRIOR_SD
    return float(-0.5 * np.sum(z * z) - np.sum(np.log(PRIOR_SD)) - np.log(2.0 * np.pi))


def prior_draws(series, seed):
    rng = np.random.default_rng(seed)
    base = np.array(base_params().flattenParams())
    out = []
    for _ in range(series):
        th = base.copy()
        th[list(FREE)] = PRIOR_MEAN + PRIOR_SD * rng.standard_normal(2)
        out.append(base_params().withFlat(th))
    return out


def observations(count=T):
    t, y, _ = cases.gaussian_series(count)
    return [TimedObservation(float(a), float(b)) for a, b in zip(t, y)]


def exact(points=85, width=7.0):
    """(posterior mean[2], sd[2], log evidence) and their errors: trapezoid rule on a points x points grid over prior mean +- width sd and
    on every other point of it."""
    t, y, has = cases.gaussian_series(T)
    ax = [PRIOR_MEAN[c] + PRIOR_SD[c] * np.linspace(-width, width, points) for c in range(2)]
    base = np.array(base_params().flattenParams())
    lj = np.zeros((points, points))
    for i, a in enumerate(ax[0]):
        for j, b in enumerate(ax[1]):
            th = base.copy()
            th[list(FREE)] = (a, b)
            ll = gr.kalman(gr.spec_of(unparam().run(base_params().withFlat(th))), t, y, has)[0][-1]
            lj[i, j] = ll + log_prior(th)

    def moments(step):
        a, b, l = ax[0][::step], ax[1][::step], lj[::step, ::step]
        wa, wb = np.full(len(a), a[1] - a[0]), np.full(len(b), b[1] - b[0])
        wa[[0, -1]] *= 0.5; wb[[0, -1]] *= 0.5
        m = l.max()
        p = np.exp(l - m) * wa[:, None] * wb[None, :]
        z = p.sum()
        ma, mb = (p.sum(axis=1) @ a) / z, (p.sum(axis=0) @ b) / z
        va, vb = (p.sum(axis=1) @ (a - ma) ** 2) / z, (p.sum(axis=0) @ (b - mb) ** 2) / z
        return np.array([ma, mb, np.sqrt(va), np.sqrt(vb), m + np.log(z)])

    fine, coarse = moments(1), moments(2)
    return fine, np.abs(fine - coarse)


def statistics(smc: SMC2, states):
    theta, w = smc.posterior()
    x = theta[:, list(FREE)]
    m = w @ x
    sd = np.sqrt(w @ (x - m) ** 2)
    return np.array([m[0], m[1], sd[0], sd[1], states[-1].log_evidence])


def never_reweighted_evidence(series, seed):
    """The evidence a run reports that never reweights: sum_t log mean_k exp(inc_t,k) of a run without rejuvenation."""
    with SMC2(unparam(), prior_draws(series, seed), N, log_prior=log_prior, free=FREE, ess_fraction=0.0, seed=seed,
              engine=OracleEngine(cases.linear_model(), N, series)) as smc:
        states = smc.run(observations())
    lw = np.array([np.zeros(series)] + [s.logw for s in states])
    return float(sum(logsumexp(lw[i + 1] - lw[i]) - np.log(series) for i in range(len(states))))


def truth_run(make_engine, seed):
    with SMC2(unparam(), prior_draws(S, seed), N, log_prior=log_prior, free=FREE, seed=seed, engine=make_engine()) as smc:
        states = smc.run(observations())
        return statistics(smc, states), sum(s.resampled for s in states)


def check_truth(runs, label):
    """runs [R, 5]; prints every z before it asserts."""
    ref, err = exact_cached()
    rms, mx, _ = zscore(runs[:, None, :], ref[None, :], err[None, :])
    z = (runs.mean(axis=0) - ref) / np.sqrt(runs.var(axis=0, ddof=1) / len(runs) + (3.0 * err) ** 2)
    print(f"    {label}: truth {np.round(ref, 5).tolist()} err {err.tolist()} replicate mean {np.round(runs.mean(axis=0), 5).tolist()} z {np.round(z, 2).tolist()}")
    assert accepted(np.sqrt(np.mean(rms ** 2)), mx.max()), (label, z.tolist())
    return z


_EXACT = []


def exact_cached():
    if not _EXACT:
        _EXACT.append(exact())
    return _EXACT[0]


def all_statistics_accepted(runs, ref, err):
    rms, mx, _ = zscore(runs[:, None, :], ref[None, :], err[None, :])
    return accepted(np.sqrt(np.mean(rms ** 2)), mx.max())


def test_the_quadrature_is_converged():
    ref, err = exact_cached()
    assert (err < 1e-6).all(), err.tolist()
    assert abs(ref[0] - PRIOR_MEAN[0]) > 0.1          # the data move the posterior: the power check below has something to reject


def test_smc2_recovers_the_exact_posterior_and_evidence():
    runs, rej = [], []
    for r in range(R):
        st, n_rej = truth_run(lambda: OracleEngine(cases.linear_model(), N, S), SEED0 + r)
        runs.append(st); rej.append(n_rej)
    runs = np.array(runs)
    print(f"    rejuvenations per replicate: {rej}")
    assert min(rej) >= 1
    check_truth(runs, "smc2 / oracle")
    ref, err = exact_cached()
    # power: the prior's moments offered as the truth are rejected ...
    prior = ref.copy()
    prior[:4] = [PRIOR_MEAN[0], PRIOR_MEAN[1], PRIOR_SD[0], PRIOR_SD[1]]
    assert not all_statistics_accepted(runs, prior, err)
    # ... and so is the evidence of a run that never reweights, held to the exact evidence
    flat = np.array([never_reweighted_evidence(S, SEED0 + r) for r in range(R)])
    rms, mx, _ = zscore(flat[:, None, None], ref[None, 4:], err[None, 4:])
    print(f"    never reweighted: evidence {np.round(flat.mean(), 4)} against {np.round(ref[4], 4)}, z {np.round(mx, 2).tolist()}")
    assert not accepted(rms, mx)


# ------------------------------------------------------------------------------------------------ algebraic checks
SA, NA, TA = 24, 32, 10


def small(seed=7, series=SA, draws=None, **kw):
    draws = prior_draws(series, seed) if draws is None else draws
    kw.setdefault("log_prior", log_prior)
    kw.setdefault("free", FREE)
    eng = OracleEngine(cases.linear_model(), NA, len(draws))
    return SMC2(unparam(), draws, NA, seed=seed, engine=eng, **kw), eng


def same(a: Smc2State, b: Smc2State):
    return (a.t == b.t and np.array_equal(a.theta, b.theta) and np.array_equal(a.logw, b.logw) and a.ess == b.ess and
            a.log_evidence == b.log_evidence and a.resampled == b.resampled and a.accepted == b.accepted)


def test_without_rejuvenation_the_evidence_is_the_mean_likelihood_exactly():
    smc, _ = small(ess_fraction=0.0)
    theta0 = smc.theta.copy()
    states = smc.run(observations(TA))
    assert not any(s.resampled for s in states) and all(np.array_equal(s.theta, theta0) for s in states)
    t, y, has = cases.gaussian_series(TA)
    keys = smc._keys(0)
    ll = np.array([oracle.OraclePf(unparam().run(p).descriptor(), NA, keys[k]).filter(t, y, has)[0] for k, p in enumerate(prior_draws(SA, 7))])
    assert np.array_equal(states[-1].logw, ll)
    assert states[-1].log_evidence == logsumexp(ll) - np.log(SA)          # exactly: the driver's closed form is this expression
    smc.close()


def test_rejuvenation_at_every_step_completes_with_zero_log_weights():
    smc, eng = small(ess_fraction=1.01, moves=2)
    states = smc.run(observations(TA))
    assert all(s.resampled for s in states) and smc.rejuvenations == TA and eng.clones == TA
    assert all((s.logw == 0.0).all() for s in states)
    assert all(0 <= s.accepted <= SA * 2 for s in states) and sum(s.accepted for s in states) > 0
    assert eng.adoptions == sum(s.accepted for s in states)
    smc.close()


@pytest.mark.parametrize("ess_fraction", [0.5, 1.01])
def test_two_runs_with_one_seed_are_bit_equal(ess_fraction):
    out = []
    for _ in range(2):
        smc, _ = small(ess_fraction=ess_fraction)
        out.append(smc.run(observations(TA)))
        smc.close()
    assert all(same(a, b) for a, b in zip(*out))


def test_only_the_free_component_moves():
    smc, _ = small(ess_fraction=1.01, free=(3,))
    start = smc.theta.copy()
    states = smc.run(observations(TA))
    assert sum(s.accepted for s in states) > 0
    fixed = [0, 1, 2]
    for s in states:   # every row is a resampled starting row in the fixed components, and moves in the free one only
        assert all(any(np.array_equal(row[fixed], r0[fixed]) for r0 in start) for row in s.theta)
    assert not all(any(row[3] == r0[3] for r0 in start) for row in states[-1].theta)
    smc.close()


def test_a_refused_proposal_is_never_accepted():
    calls = []

    def wall(theta):            # -inf for every vector but the starting ones
        known = any(np.array_equal(theta, r) for r in start)
        calls.append(known)
        return 0.0 if known else -np.inf

    draws = prior_draws(SA, 7)
    start = np.array([p.flattenParams() for p in draws])
    smc, eng = small(draws=draws, ess_fraction=1.01, log_prior=wall)
    states = smc.run(observations(TA))
    assert all(s.accepted == 0 for s in states) and eng.adoptions == 0 and not all(calls)
    assert all(any(np.array_equal(row, r0) for r0 in start) for row in states[-1].theta)
    smc.close()


def test_a_theta_the_model_refuses_is_rejected():
    class Picky:                # unparam.run refuses every parameter tree but the starting ones
        def __init__(self, inner, rows):
            self.inner, self.rows, self.refused = inner, rows, 0

        def run(self, p):
            if not any(np.array_equal(p.flattenParams(), r) for r in self.rows):
                self.refused += 1
                raise ValueError("refused")
            return self.inner.run(p)

    draws = prior_draws(SA, 7)
    picky = Picky(unparam(), np.array([p.flattenParams() for p in draws]))
    eng = OracleEngine(cases.linear_model(), NA, SA)
    smc = SMC2(picky, draws, NA, log_prior=log_prior, free=FREE, ess_fraction=1.01, seed=7, engine=eng)
    states = smc.run(observations(TA))
    assert picky.refused > 0 and all(s.accepted == 0 for s in states) and eng.adoptions == 0
    smc.close()


def dead_draws():
    draws = prior_draws(SA, 7)
    th = np.array(draws[5].flattenParams())
    th[0] = -400.0              # an observation sd of e^-400: every log-weight of that series is -inf at the first datum
    draws[5] = base_params().withFlat(th)
    return draws


def test_a_dead_series_is_masked_and_replaced_at_the_next_resampling():
    smc, eng = small(draws=dead_draws(), ess_fraction=0.5)
    obs = observations(TA)
    first = smc.step(obs[0])
    assert first.logw[5] == -np.inf and not smc.active[5] and np.isfinite(np.delete(first.logw, 5)).all()
    states = [first]
    for o in obs[1:]:
        before = smc.active.copy()
        states.append(smc.step(o))
        if states[-1].resampled:
            assert smc.active.all() and np.isfinite(states[-1].logw).all() and not (smc.theta[:, 0] == -400.0).any()
            break
        assert not smc.active[5] and np.array_equal(before, smc.active) and states[-1].logw[5] == -np.inf
    assert states[-1].resampled, "no resampling within the series: the case shows nothing"
    assert np.isfinite(smc.step(obs[len(states)]).log_evidence)
    smc.close()


def test_all_series_dead_raises():
    smc, _ = small(ess_fraction=0.5)
    smc.step(observations(2)[0])
    with pytest.raises(RuntimeError, match="every parameter particle is dead"):
        smc.step(TimedObservation(1.0, 1e200))
    smc.close()


def test_systematic_ancestors_never_choose_a_zero_weight():
    w = np.array([0.0, 0.5, 0.0, 0.5])
    for u in (0.0, 0.25, 0.999):
        assert set(systematic_ancestors(w, u).tolist()) == {1, 3}
