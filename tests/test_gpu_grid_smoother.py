"""cssm_pf_interpolate against the exact fixed-interval smoother (tests/grid_reference.py: `rts`, the grid smoother): a truth that
shares neither code nor variates with the kernels or the oracle.  tests/test_interpolate.py and tests/test_gpu_fleet_interpolate.py
hold the kernels to the oracle bit for bit; tests/test_grid_smoother.py proves the references and holds the oracle to them; here the
handle itself is held to them at N well beyond one tile, with the resamplers the oracle's interpolate does not have.

One NativePf per case, reseeded SEED0 + r for R replicates (fixed seeds, no retries: a case passes or fails deterministically),
T = 12 with the removed observations of test_interpolate's _series.  Per statistic (mean, lower, upper, and the eta quantiles where
a closed form or a monotone link gives them) and component, over ALL T+1 rows: z = (replicate mean - truth) / sqrt(s^2 / R +
(3 err)^2) has an RMS <= 3 and a maximum <= 8.  The same runs must REJECT the filtering means and the truth shifted by one row in
either direction.  The returned ll goes through test_gpu_grid_reference's check_ll against the grid filter's.
"""
import time

import numpy as np
import pytest

from test_gpu_grid_reference import HEADER, check_ll
from test_grid_smoother import (SMOOTHER_CASES, T, check_eta_of_mean, check_power, check_smoothing, gaussian_truth, accepted,
                                smoother_case, stack, truth_of, zscore)
import grid_reference as gr

pytestmark = pytest.mark.gpu

R = 16
SEED0 = 93000
N = 1 << 18


def replicates(name, n, r_count, resampler=0, pairing=False):
    """R interpolations of one handle, reseeded SEED0 + r: (ll[R], stacked summaries); eta_of_mean is checked on every one."""
    from composablestatespacemodels_amd.filter import NativePf
    model, t, y, has = smoother_case(name)
    g = NativePf(model, n, SEED0)
    outs = []
    t_start = time.perf_counter()
    try:
        if resampler:
            g.set_option(2, resampler)                         # CSSM_OPT_RESAMPLER: 1 stratified, 2 multinomial
        for r in range(r_count):
            g.reseed(SEED0 + r)
            outs.append(g.interpolate(t, y, has, 0.975, pairing))
            check_eta_of_mean(model, t, outs[-1][1], outs[-1][4])
    finally:
        g.close()
    print(f"\n{name}: N = {n}, R = {r_count}, resampler {resampler}, pairing {pairing}: {time.perf_counter() - t_start:.2f} s on the device path")
    return np.array([o[0] for o in outs]), stack(outs)


def grid_of(name):
    """The grid filter's likelihood of the case (the forward pass of the smoother for the grid cases)."""
    tr = truth_of(name)
    if tr.grid is not None:
        return tr.grid
    model, t, y, has = smoother_case(name)
    return gr.reference(model, t, y, has)


@pytest.mark.parametrize("name", list(SMOOTHER_CASES))
def test_interpolation_matches_the_smoother(name):
    tr = truth_of(name)
    lls, runs = replicates(name, N, R)
    check_smoothing(name, runs, tr)
    check_power(name, runs[0], tr)
    print(HEADER)
    check_ll(name, N, lls, grid_of(name))


@pytest.mark.parametrize("kind,label", [(1, "stratified"), (2, "multinomial")])
def test_native_resamplers_interpolate_to_the_smoother(kind, label):
    """launch_resample under cssm_pf_interpolate with the two resamplers the oracle's interpolate does not have: their ancestors
    land in the history the lineages are composed from."""
    tr = truth_of("c2")
    lls, runs = replicates("c2", N, R, resampler=kind)
    check_smoothing(f"c2 {label}", runs, tr)
    check_power(f"c2 {label}", runs[0], tr)
    print(HEADER)
    check_ll(f"c2 {label}", N, lls, grid_of("c2"))


@pytest.mark.parametrize("n", [(1 << 20) + 77, 1 << 22])
def test_large_and_odd_n_interpolate_to_the_smoother(n):
    """An N that is no multiple of the tile, and the wave-sum path of d <= 2 beyond 2^20 (a history of 13 clouds of 2^22)."""
    tr = truth_of("c1")
    _, runs = replicates("c1", n, 8)
    check_smoothing(f"c1 N={n}", runs, tr, eta=False)
    check_power(f"c1 N={n}", runs[0], tr)


def test_reference_pairing_against_the_smoother():
    """reference_pairing: output row o holds the smoothed state of row T - o, and its eta the time of index o -- gbsg's seasonal
    H(t) makes that time matter: gamma = H(time of index o) . x_{T-o} in closed form."""
    model, t, y, has = smoother_case("gbsg")
    paired, plain = gaussian_truth(model, t, y, has, pairing=True), truth_of("gbsg")
    np.testing.assert_array_equal(paired.mean, plain.mean[::-1])
    assert not np.allclose(paired.eta_lo, plain.eta_lo[::-1], rtol=0, atol=1e-3)      # the time of the index matters
    _, runs = replicates("gbsg", N, R, pairing=True)
    check_smoothing("gbsg paired", runs, paired)
    for what, x, ref in (("mean", runs[0], plain.mean), ("eta_lower", runs[3][:, :, None], plain.eta_lo[:, None])):
        rms, mx, _ = zscore(x, ref, np.zeros_like(ref))
        print(f"    gbsg paired power, unreversed {what:9}: z rms {np.round(rms, 1).tolist()}  max {np.round(mx, 1).tolist()}")
        assert not accepted(rms, mx), f"the unreversed {what} is not rejected"
    assert T % 2 == 0                                            # (row T / 2 pairs with itself: the rejection rests on the others)
