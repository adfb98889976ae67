"""The smoothed rows of interpolate against an exact fixed-interval smoother (tests/grid_reference.py: `rts` in closed form for the
Gaussian-observation models, a backward pass over the grid filter's grids for the others).  Neither shares code, variates or an
elementary function with the kernels or the oracle, so what the oracle and the kernels state together -- which cloud row s
summarises, how the ancestors compose backwards -- is judged from outside: row 0 is the initial cloud, row s+1 the cloud at t[s]
traced back from the end, and as N grows row s converges to p(x_s | y_1..T).

* the references are proven first: the grid smoother against `rts` (d = 1 and d = 3), `rts` against the Kalman filter, the grid
  smoother's refinement bounds and its last row against the grid filter;
* the premise of the power checks, from the references alone: on the rows of the removed observations smoothing differs from
  filtering, and from itself one row later, by more than 10 x the smoother's own error bound;
* the CPU oracle at N = 2^16 with 16 seeds: z = (replicate mean - truth) / sqrt(s^2 / R + (3 err)^2) per statistic (mean, lower,
  upper) and component over ALL T+1 rows has an RMS <= 3 and a maximum <= 8 (the criteria of test_gpu_grid_reference's
  check_filtering); the same runs REJECT the filtering means and the truth shifted by one row in either direction.

The order statistic of floor(0.975 N) against the 97.5 % quantile is O(1 / N) off: no correction at these N.
tests/test_gpu_grid_smoother.py holds the kernels to the same truths with the helpers of this file.
"""
from dataclasses import dataclass

import numpy as np
import pytest
from scipy.special import ndtri

import cases
import grid_reference as gr
from oracle import oracle

T = 12
GAP = slice(T // 3, T // 3 + max(2, T // 5))                # the removed observations of tests/test_interpolate.py::_series

# name: (model, Gaussian series or Poisson counts)
SMOOTHER_CASES = {
    "linear": (cases.linear_model, True),
    "gbsg": (cases.gen_brownian_seasonal_gaussian, True),
    "c1": (cases.c1_model, False),
    "c2": (cases.c2_model, False),
    "negbin": (cases.negbin_model, False),
    "studentt": (cases.studentt_model, True),
}
GAUSSIAN = ("linear", "gbsg")


def smoother_case(name):
    mk, gaussian = SMOOTHER_CASES[name]
    t, y, has = cases.gaussian_series(T) if gaussian else cases.poisson_counts(T)
    has = has.copy()
    has[GAP] = 0
    return mk(), t, y, has


def row_times(t):
    """The time of output index k: min(t) for the initial cloud, t[k - 1] after."""
    return np.concatenate([[np.min(t)], t])


def link(obs, g):
    return np.exp(g) if obs in ("poisson", "negbin", "zip") else g


@dataclass
class Truth:
    mean: np.ndarray                # [T+1, d] smoothed means, 2.5 % and 97.5 % quantiles and their error bounds
    lo: np.ndarray
    hi: np.ndarray
    mean_err: np.ndarray
    lo_err: np.ndarray
    hi_err: np.ndarray
    filt_mean: np.ndarray           # [T, d] FILTERING means at t[0..T): what smoothing must be told apart from
    filt_err: np.ndarray
    eta_lo: np.ndarray              # [T+1] quantiles of eta at the row's own time, or None (d > 1 under a non-Gaussian model)
    eta_hi: np.ndarray
    eta_lo_err: np.ndarray
    eta_hi_err: np.ndarray
    grid: object                    # the grid filter's result (ll, ll_err), None for the closed form


_TRUTH = {}


def gaussian_truth(model, t, y, has, pairing=False):
    """`rts` as a Truth.  With pairing, output row o holds state row T - o and eta = H(time of index o) . x_{T-o}."""
    spec = gr.spec_of(model)
    ms, Ps = gr.rts(spec, t, y, has)
    _, km, kv = gr.kalman(spec, t, y, has)
    if pairing:
        ms, Ps = ms[::-1], Ps[::-1]
    sd = np.sqrt(np.einsum("sii->si", Ps))
    gm = np.array([gr.gamma_moments(spec, ms[k], Ps[k], time) for k, time in enumerate(row_times(t))])
    z = np.zeros_like(ms)
    zz = np.zeros(len(ms))
    return Truth(ms, ms + ndtri(0.025) * sd, ms + ndtri(0.975) * sd, z, z, z, km, np.zeros_like(km),
                 gm[:, 0] + ndtri(0.025) * gm[:, 1], gm[:, 0] + ndtri(0.975) * gm[:, 1], zz, zz, None)


def truth_of(name) -> Truth:
    if name not in _TRUTH:
        model, t, y, has = smoother_case(name)
        if name in GAUSSIAN:
            _TRUTH[name] = gaussian_truth(model, t, y, has)
        else:
            g = gr.smoother_reference(model, t, y, has)
            f = g.filter
            el = eh = ele = ehe = None
            if g.mean.shape[1] == 1:                           # gamma = x is monotone in x: the quantiles go through the link
                obs = gr.spec_of(model).obs
                lo, hi = g.lo[:, 0], g.hi[:, 0]
                el, eh = link(obs, lo), link(obs, hi)
                ele = np.maximum(np.abs(link(obs, lo + g.lo_err[:, 0]) - el), np.abs(link(obs, lo - g.lo_err[:, 0]) - el))
                ehe = np.maximum(np.abs(link(obs, hi + g.hi_err[:, 0]) - eh), np.abs(link(obs, hi - g.hi_err[:, 0]) - eh))
            _TRUTH[name] = Truth(g.mean, g.lo, g.hi, g.mean_err, g.lo_err, g.hi_err, f.mean, f.mean_err, el, eh, ele, ehe, f)
    return _TRUTH[name]


# --------------------------------------------------------------------------------------------- the criteria
def zscore(x, ref, err):
    """x [R, rows, d] replicates against ref [rows, d] known to err: (rms, max) per component over the rows."""
    m, s = x.mean(axis=0), x.std(axis=0, ddof=1)
    z = (m - ref) / np.sqrt(s * s / x.shape[0] + (3.0 * err) ** 2 + 1e-300)
    return np.sqrt(np.mean(z * z, axis=0)), np.max(np.abs(z), axis=0), np.argmax(np.abs(z), axis=0)


def accepted(rms, mx):
    return bool(np.all(rms <= 3.0) and np.all(mx <= 8.0))


def check_smoothing(label, runs, tr: Truth, eta=True):
    """runs: the replicates' (mean, lower, upper [R, T+1, d], eta_lower, eta_upper [R, T+1]).  Every row, every component."""
    stats = [("mean", runs[0], tr.mean, tr.mean_err), ("lower", runs[1], tr.lo, tr.lo_err), ("upper", runs[2], tr.hi, tr.hi_err)]
    if eta and tr.eta_lo is not None:
        stats += [("eta_lower", runs[3][:, :, None], tr.eta_lo[:, None], tr.eta_lo_err[:, None]),
                  ("eta_upper", runs[4][:, :, None], tr.eta_hi[:, None], tr.eta_hi_err[:, None])]
    bad = []
    for name, x, ref, err in stats:
        assert x.shape[1:] == ref.shape
        rms, mx, at = zscore(x, ref, err)
        print(f"    {label} {name:9}: z rms per component {np.round(rms, 2).tolist()}  max {np.round(mx, 2).tolist()} at row {at.tolist()}")
        if not accepted(rms, mx):
            bad.append(f"{name} (rms {rms}, max {mx})")
    assert not bad, f"{label}: smoothed rows off the smoother: " + "; ".join(bad)


def check_power(label, means, tr: Truth):
    """The same replicate means, the same criteria: the filtering means (rows 1..T) and the truth shifted by one row in either
    direction must be REJECTED."""
    for what, x, ref, err in (("filtering means", means[:, 1:], tr.filt_mean, tr.filt_err),
                              ("truth one row later", means[:, :-1], tr.mean[1:], tr.mean_err[1:]),
                              ("truth one row earlier", means[:, 1:], tr.mean[:-1], tr.mean_err[:-1])):
        rms, mx, _ = zscore(x, ref, err)
        print(f"    {label} power, {what:21}: z rms {np.round(rms, 1).tolist()}  max {np.round(mx, 1).tolist()}")
        assert not accepted(rms, mx), f"{label}: {what} are not rejected (rms {rms}, max {mx})"


def check_eta_of_mean(model, t, mean, eta_of_mean):
    """eta_of_mean == link(H(time of the output index) . returned mean)."""
    spec = gr.spec_of(model)
    want = [link(spec.obs, float(spec.H(float(time)) @ mean[k])) for k, time in enumerate(row_times(t))]
    np.testing.assert_allclose(eta_of_mean, want, rtol=1e-12, atol=0)


# --------------------------------------------------------------------------------------------- the references, proven
@pytest.mark.parametrize("name", GAUSSIAN)
def test_grid_smoother_matches_rts(name):
    model, t, y, has = smoother_case(name)
    ms, Ps = gr.rts(gr.spec_of(model), t, y, has)
    sd = np.sqrt(np.einsum("sii->si", Ps))
    g = gr.smoother_reference(model, t, y, has)
    print(f"\n{name}: |dmean| {np.abs(g.mean - ms).max():.2e}  |dlo| {np.abs(g.lo - (ms + ndtri(0.025) * sd)).max():.2e}  "
          f"|dhi| {np.abs(g.hi - (ms + ndtri(0.975) * sd)).max():.2e}  points {g.filter.points}")
    np.testing.assert_allclose(g.mean, ms, rtol=0, atol=1e-8)
    for q, got, err in ((0.025, g.lo, g.lo_err), (0.975, g.hi, g.hi_err)):
        assert np.all(np.abs(got - (ms + ndtri(q) * sd)) <= err)


@pytest.mark.parametrize("name", GAUSSIAN)
def test_rts_against_the_kalman_filter(name):
    model, t, y, has = smoother_case(name)
    spec = gr.spec_of(model)
    ms, Ps = gr.rts(spec, t, y, has)
    _, km, kv = gr.kalman(spec, t, y, has)
    assert ms.shape == (T + 1, spec.d) and Ps.shape == (T + 1, spec.d, spec.d)
    np.testing.assert_allclose(ms[-1], km[-1], rtol=0, atol=1e-12)                 # nothing after the last datum
    np.testing.assert_allclose(np.diag(Ps[-1]), kv[-1], rtol=0, atol=1e-12)
    assert t[0] == np.min(t)
    np.testing.assert_allclose(ms[0], ms[1], rtol=0, atol=1e-12)                   # dt = 0: the identity transition
    np.testing.assert_allclose(Ps[0], Ps[1], rtol=0, atol=1e-12)
    # no observation at all: the prior pushed through the transitions, smoothing changes nothing
    m0, P0 = gr.rts(spec, t, y, np.zeros(T, dtype=np.uint8))
    m, v, now = spec.m0.copy(), spec.c0.copy(), float(t[0])
    for s in range(T):
        if t[s] != now:
            A, b, q = spec.transition(float(t[s]) - now)
            m, v, now = A * m + b, A * A * v + q, float(t[s])
        np.testing.assert_allclose(m0[s + 1], m, rtol=0, atol=1e-12)
        np.testing.assert_allclose(P0[s + 1], np.diag(v), rtol=0, atol=1e-12)
    # the smoothed variance never exceeds the filtering variance
    assert np.all(np.einsum("sii->si", Ps)[1:] <= kv + 1e-14)


@pytest.mark.parametrize("name", ["c1", "c2", "negbin", "studentt"])
def test_grid_smoother_is_refined_enough(name):
    model, t, y, has = smoother_case(name)
    g = gr.smoother_reference(model, t, y, has)
    f = gr.reference(model, t, y, has)
    print(f"\n{name}: d = {g.mean.shape[1]}  mean_err {g.mean_err.max():.2e}  lo_err {g.lo_err.max():.2e}  hi_err {g.hi_err.max():.2e}  "
          f"|last row - filter| {np.abs(g.mean[-1] - f.mean[-1]).max():.2e}  points {g.filter.points}")
    assert g.mean_err.max() <= 1e-4 and g.lo_err.max() <= 1e-3 and g.hi_err.max() <= 1e-3
    np.testing.assert_allclose(g.mean[-1], f.mean[-1], rtol=0, atol=1e-10)
    # the forward pass the smoother keeps IS the grid filter
    np.testing.assert_array_equal(g.filter.ll_t, f.ll_t)
    np.testing.assert_array_equal(g.filter.mean, f.mean)
    np.testing.assert_array_equal(g.filter.ll_err, f.ll_err)


def test_grid_smoother_refuses_the_lgcp():
    t, y, has = cases.event_times(5)
    with pytest.raises(ValueError):
        gr.grid_smoother(gr.spec_of(cases.c4_model()), t, y, has)


@pytest.mark.parametrize("name", list(SMOOTHER_CASES))
def test_smoothing_differs_from_filtering_and_from_its_neighbour_on_the_gap(name):
    """What the power checks rest on, from the references alone."""
    tr = truth_of(name)
    rows = np.arange(T + 1)[1:][GAP]                            # the output rows of the removed observations
    for k in rows:
        bound = 10.0 * np.maximum(tr.mean_err[k], tr.mean_err[k + 1]) + 1e-12
        d_filter = np.abs(tr.mean[k] - tr.filt_mean[k - 1])
        d_next = np.abs(tr.mean[k] - tr.mean[k + 1])
        print(f"    {name} row {k}: |smoothed - filtered| {d_filter.tolist()}  |smoothed - next row| {d_next.tolist()}  10 err {bound.tolist()}")
        assert np.any(d_filter > bound) and np.any(d_next > bound)


# --------------------------------------------------------------------------------------------- the oracle against the truth
ORACLE_N, ORACLE_R = 1 << 16, 16


def stack(outs):
    """[(ll, mean, lower, upper, eta_of_mean, eta_lower, eta_upper)] -> (mean, lower, upper [R, T+1, d], eta_lower, eta_upper [R, T+1])."""
    return [np.array([o[k] for o in outs]) for k in (1, 2, 3, 5, 6)]


@pytest.mark.parametrize("name", ["linear", "gbsg", "c1", "c2"])
def test_oracle_interpolation_converges_to_the_smoother(name):
    model, t, y, has = smoother_case(name)
    tr = truth_of(name)
    o = oracle.OraclePf(model.descriptor(), ORACLE_N, 1)
    outs = []
    for r in range(ORACLE_R):
        o.reseed(7000 + r)
        outs.append(o.interpolate(t, y, has))
        check_eta_of_mean(model, t, outs[-1][1], outs[-1][4])
    runs = stack(outs)
    print(f"\n{name}: oracle N = {ORACLE_N}, R = {ORACLE_R}")
    check_smoothing(name, runs, tr)
    check_power(name, runs[0], tr)
