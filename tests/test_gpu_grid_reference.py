"""The HIP filters against the exact grid-filter answer (tests/grid_reference.py): a truth that shares neither code nor variates
with the kernels, and does not depend on N.

Every case runs R replicate seeds (NativePf.reseed, fixed seeds, no retries: the runs are bit-reproducible, so each case passes or
fails deterministically) and asserts
* |mean(ll) - ll_grid| <= 4.5 s / sqrt(R) + 3 grid_err + s^2 / 2, s the replicate sd of ll (s^2 / 2: the Jensen bias of the log of
  an unbiased estimate);
* for the streamed cases, the replicate means of summary()'s state_mean and interval ends against the grid's filtering mean and
  2.5 % / 97.5 % quantiles, per component: z = (mean - grid) / sqrt(s^2 / R + (3 err)^2) has an RMS over the observations <= 3
  and a maximum <= 8 (t with R - 1 degrees of freedom, a few hundred of them per case);
* the power check: the same N and seeds on the model with one parameter moved by a stated amount are REJECTED by the unperturbed
  grid (|mean(ll') - ll_grid| above its own margin) -- a tolerance that accepts everything fails;
* for the main cases, s(N/16) / s(N) in [2.2, 7]: a bug that inflates the variance cannot widen its own tolerance.
"""
import math

import numpy as np
import pytest

import grid_reference as gr
from test_grid_reference import CASES, case, grid_of, perturbed

pytestmark = pytest.mark.gpu

R = 8
SEED0 = 91000
HEADER = (f"{'case':16} {'N':>9} {'R':>2} {'mean ll':>14} {'grid ll':>14} {'grid_err':>9} {'s':>9} {'margin':>9} {'dev':>10} "
          f"{'power |dev|/margin':>18}")


def replicates(model, n, t, y, has, prec=0, stream=False, resampler=0):
    """R runs reseeded SEED0 + r: ll[R] and, streamed, the summaries [R, T, d] (mean, lower, upper)."""
    from composablestatespacemodels_amd.filter import NativePf
    g = NativePf(model, n, SEED0, lgcp_precision=prec)
    if resampler:
        g.set_option(2, resampler)                         # CSSM_OPT_RESAMPLER: 1 stratified, 2 multinomial
    lls, summ = [], []
    try:
        for r in range(R):
            g.reseed(SEED0 + r)
            if not stream:
                lls.append(g.run(t, y, has)[0])
                continue
            g.init(float(np.min(t)))
            rows = []
            for s in range(len(t)):
                ll, _ = g.step(float(t[s]), float(y[s]) if has[s] else None, bool(has[s]))
                m, lo, hi = g.summary(0.975)[:3]
                rows.append((m, lo, hi))
            lls.append(ll)
            summ.append(rows)
    finally:
        g.close()
    out = np.array(lls)
    if not stream:
        return out, None
    return out, [np.array([[row[k] for row in rep] for rep in summ]) for k in range(3)]


def margin_of(lls, grid_err):
    s = float(np.std(lls, ddof=1))
    return s, 4.5 * s / math.sqrt(len(lls)) + 3.0 * grid_err + s * s / 2.0


def check_ll(label, n, lls, g, power=None):
    s, margin = margin_of(lls, float(g.ll_err[-1]))
    dev = float(np.mean(lls) - g.ll)
    ptxt = ""
    if power is not None:
        sp, mp = margin_of(power, float(g.ll_err[-1]))
        ptxt = f"{abs(float(np.mean(power)) - g.ll) / mp:18.2f}"
    print(f"{label:16} {n:9d} {len(lls):2d} {np.mean(lls):14.8f} {g.ll:14.8f} {g.ll_err[-1]:9.2e} {s:9.2e} {margin:9.2e} {dev:+10.2e} {ptxt}")
    assert g.ll_err[-1] <= margin / 10, "the grid is not refined enough for this tolerance"
    assert abs(dev) <= margin, f"{label}: mean ll {np.mean(lls)} vs grid {g.ll} (margin {margin})"
    if power is not None:
        assert abs(float(np.mean(power)) - g.ll) > mp, f"{label}: the perturbed model is not rejected"


def check_filtering(label, summ, g):
    for k, (name, ref, err) in enumerate((("mean", g.mean, g.mean_err), ("lower", g.lo, g.lo_err), ("upper", g.hi, g.hi_err))):
        x = summ[k]                                             # [R, T, d]
        m, s = x.mean(axis=0), x.std(axis=0, ddof=1)
        z = (m - ref) / np.sqrt(s * s / x.shape[0] + (3.0 * err) ** 2 + 1e-300)
        rms, mx = np.sqrt(np.mean(z * z, axis=0)), np.max(np.abs(z), axis=0)
        print(f"    {label} {name:5}: z rms per component {np.round(rms, 2).tolist()}  max {np.round(mx, 2).tolist()} "
              f"at step {np.argmax(np.abs(z), axis=0).tolist()}")
        assert np.all(rms <= 3.0) and np.all(mx <= 8.0), f"{label}: filtering {name} off the grid (rms {rms}, max {mx})"


STREAMED = ["c1", "c1_ou", "c1_gen", "euler", "linear", "negbin", "zip", "bernoulli", "studentt", "beta", "c2", "studentt_outlier",
            "lgcp_seasonal"]


@pytest.mark.parametrize("name", STREAMED)
def test_filter_matches_the_grid(name):
    """Every SDE kind x Poisson, every observation model, C2 with missing data, an observation redone relative to the max, the seasonal LGCP: N = 2^20,
    likelihood and filtering distributions, and the power check."""
    model, t, y, has, prec = case(name)
    idx, amount, what = CASES[name][3]
    n = 1 << 20
    g = grid_of(name)
    lls, summ = replicates(model, n, t, y, has, prec, stream=True)
    power, _ = replicates(perturbed(model, idx, amount), n, t, y, has, prec)
    print(f"\n{HEADER}\n(power check: {what})")
    check_ll(name, n, lls, g, power)
    check_filtering(name, summ, g)


@pytest.mark.parametrize("name", ["c1", "c2", "linear"])
def test_replicate_sd_shrinks_like_one_over_sqrt_n(name):
    model, t, y, has, prec = case(name)
    s_small = float(np.std(replicates(model, 1 << 16, t, y, has, prec)[0], ddof=1))
    s_big = float(np.std(replicates(model, 1 << 20, t, y, has, prec)[0], ddof=1))
    print(f"\n{name}: s(2^16) = {s_small:.3e}  s(2^20) = {s_big:.3e}  ratio {s_small / s_big:.2f}")
    assert 2.2 <= s_small / s_big <= 7.0


@pytest.mark.parametrize("name,n", [("c1", (1 << 20) + 77), ("c1", 1 << 22), ("c1", 1 << 24), ("c2", 1 << 22), ("c4", 1 << 24)])
def test_large_n_default_paths_match_the_grid(name, n):
    """Paths that exist only at large N (wave sums at d <= 2 beyond 2^20, group sums, LGCP at 2^24), checked only GPU against GPU
    before: here against the grid."""
    model, t, y, has, prec = case(name)
    g = grid_of(name)
    lls, _ = replicates(model, n, t, y, has, prec)
    power = None
    if name == "c4":
        idx, amount, what = CASES[name][3]
        power, _ = replicates(perturbed(model, idx, amount), n, t, y, has, prec)
    print(f"\n{HEADER}")
    check_ll(name, n, lls, g, power)


@pytest.mark.parametrize("kind,label", [(1, "stratified"), (2, "multinomial")])
def test_native_resamplers_match_the_grid(kind, label):
    model, t, y, has, prec = case("c2")
    idx, amount, what = CASES["c2"][3]
    n = 1 << 20
    g = grid_of("c2")
    lls, _ = replicates(model, n, t, y, has, resampler=kind)
    power, _ = replicates(perturbed(model, idx, amount), n, t, y, has, resampler=kind)
    print(f"\n{HEADER}\n(power check: {what})")
    check_ll(f"c2 {label}", n, lls, g, power)


def test_residual_resampling_matches_the_grid():
    """The host `Resample[A]` seam with the residual extension: Filter(model, Resampling.residualResampling) at N = 2^16."""
    from composablestatespacemodels_amd.filter import Filter, Resampling
    from composablestatespacemodels_amd.model import TimedObservation
    model, t, y, has, prec = case("c2")
    idx, amount, what = CASES["c2"][3]
    n = 1 << 16
    g = grid_of("c2")
    data = [TimedObservation(float(a), float(b) if h else None) for a, b, h in zip(t, y, has)]

    def lls_of(m):
        return np.array([Filter(m, Resampling.residualResampling, seed=SEED0 + r).llFilter(data, n) for r in range(R)])
    print(f"\n{HEADER}\n(power check: {what})")
    check_ll("c2 residual", n, lls_of(model), g, lls_of(perturbed(model, idx, amount)))


def test_batch_chains_match_their_own_grids():
    """NativePfBatch: 4 chains at 4 parameter sets of C1's structure, each against its own grid."""
    from composablestatespacemodels_amd.filter import NativePfBatch
    base, t, y, has, _ = case("c1")
    models = [perturbed(base, 2, dl) for dl in (0.0, math.log(0.5), math.log(2.0), math.log(4.0))]
    n, B = 1 << 20, 4
    b = NativePfBatch(base, n, B)
    try:
        runs = []
        for r in range(R):
            ll, _, rc = b.filter(models, [SEED0 + 10 * r + k for k in range(B)], t, y, has, want_path=False)
            assert np.all(rc == 0)
            runs.append(ll)
        runs = np.array(runs)
    finally:
        b.close()
    print(f"\n{HEADER}")
    grids = [gr.reference(m, t, y, has) for m in models]
    for k in range(B):
        check_ll(f"batch chain {k}", n, runs[:, k], grids[k])
    # each chain is told apart from its neighbours' grids
    for k in range(B):
        s, margin = margin_of(runs[:, k], 0.0)
        others = [abs(float(np.mean(runs[:, k])) - grids[j].ll) for j in range(B) if j != k]
        assert min(others) > margin
