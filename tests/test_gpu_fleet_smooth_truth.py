"""cssm_fleet_smooth against the exact fixed-interval smoother (tests/grid_reference.py: `rts` in closed form, the grid smoother) --
the reason the call exists.  The criteria are those of tests/test_grid_smoother.py: per statistic and component, over ALL rows,
z = (replicate mean - truth) / sqrt(s^2 / R + (3 err)^2) has an rms <= 3 and a maximum <= 8.  The R replicates are R series of ONE
call, keyed SEED0 + r (fixed seeds, no retries: a case passes or fails deterministically).

Short series: the "linear", "c1" and "c2" cases of SMOOTHER_CASES (T = 12, the removed observations), N = n_traj = 4096: accepted, and
the same runs reject the filtering means and the truth shifted by a row.

Long series: "linear" on cases.gaussian_series(100), nothing removed, N = n_traj = 1000, R = 128.  cssm_fleet_smooth is accepted over all
101 rows; cssm_fleet_interpolate on the same fleet and keys is REJECTED on lower and upper (the premise is established on the CPU in
tests/test_fleet_smooth_host.py, which also says how R was chosen).  Both are judged against `rts` with the quantiles taken at the
probabilities the returned order statistics estimate (test_fleet_smooth_host.rank_truth): the O(1 / M) rank offset is 0.017 posterior
standard deviations at M = 1000 and shows at R = 128 (measured on the twin: `upper` reads z rms 1.53, max 4.98 against the plain 97.5 %
quantile, 1.08 and 3.27 against the rank's own)."""
import numpy as np
import pytest

from test_fleet_smooth_host import LONG_N, LONG_R, LONG_SEED0, long_case, rank_truth
from test_grid_smoother import accepted, check_eta_of_mean, check_power, check_smoothing, smoother_case, truth_of, zscore

pytestmark = pytest.mark.gpu

R, SEED0, N = 16, 93000, 4096


def fleet_runs(model, t, y, has, n, seeds, call, **kw):
    """the replicates as the series of one call: (ll[R], (mean, lower, upper [R, T + 1, d], eta_lower, eta_upper [R, T + 1]), rows)"""
    from composablestatespacemodels_amd.filter import NativePfFleet
    with NativePfFleet(model, n, len(seeds)) as fl:
        fl.reseed(seeds)
        ll, rows, rc = getattr(fl, call)([(t, y, has)] * len(seeds), **kw)
    assert not rc.any(), rc
    return ll, [np.array([r[q] for r in rows]) for q in (0, 1, 2, 4, 5)], rows


@pytest.mark.parametrize("name", ["linear", "c1", "c2"])
def test_short_series_match_the_smoother(name):
    model, t, y, has = smoother_case(name)
    tr = truth_of(name)
    _, runs, rows = fleet_runs(model, t, y, has, N, [SEED0 + r for r in range(R)], "smooth")
    for r in (0, R - 1):
        check_eta_of_mean(model, t, rows[r][0], rows[r][3])
    print(f"\n{name}: N = n_traj = {N}, R = {R}")
    check_smoothing(name, runs, tr)
    check_power(name, runs[0], tr)


def test_long_series_smoothing_is_accepted_where_interpolation_is_rejected():
    """Measured on an MI355X (R = 128, N = n_traj = 1000, T = 100; z rms / max over the 101 rows against rank_truth):
    smooth      mean 1.00 / 2.64   lower 1.12 / 2.71   upper 1.08 / 3.27   eta_lower 1.10 / 2.56   eta_upper 1.10 / 3.38   -- accepted
    interpolate lower 4.07 / 9.23 (row 9)   upper 3.62 / 8.57 (row 5)                                                      -- rejected
    mean width of the 95 % interval over rows 1 .. 20: smooth 1.3624, interpolate 1.1712, truth 1.3621.
    R = 128 is the count at which the CPU oracle's genealogical rows are rejected on both sides (tests/test_fleet_smooth_host.py)."""
    model, t, y, has = long_case()
    tr = rank_truth(model, t, y, has, LONG_N)
    seeds = [LONG_SEED0 + r for r in range(LONG_R)]
    print(f"\nlinear, T = {len(t)}, N = n_traj = {LONG_N}, R = {LONG_R}")
    _, runs, _ = fleet_runs(model, t, y, has, LONG_N, seeds, "smooth", n_traj=LONG_N)
    assert runs[0].shape == (LONG_R, len(t) + 1, 1)
    check_smoothing("smooth", runs, tr)
    _, gen, _ = fleet_runs(model, t, y, has, LONG_N, seeds, "interpolate")
    for name, x, ref in (("lower", gen[1], tr.lo), ("upper", gen[2], tr.hi)):
        rms, mx, at = zscore(x, ref, np.zeros_like(ref))
        print(f"    interpolate {name:5}: z rms {np.round(rms, 2).tolist()}  max {np.round(mx, 2).tolist()} at row {at.tolist()}")
        assert not accepted(rms, mx), f"interpolate's {name} is not rejected (rms {rms}, max {mx})"
    # what coalesced: the distinct values a row of the genealogy still holds show in the spread of its interval across replicates
    early = slice(1, 21)
    print(f"    width of the 95 % interval, rows 1..20, mean over replicates: smooth {np.mean(runs[2][:, early] - runs[1][:, early]):.4f}  "
          f"interpolate {np.mean(gen[2][:, early] - gen[1][:, early]):.4f}  truth {np.mean(tr.hi[early] - tr.lo[early]):.4f}")
