"""-m gpu: every kind of fleet launch at the particle counts where the block's geometry turns a corner.

A fleet's block has threads = min(512, max(64, roundup64(ceil(N / 4)))) threads (csrc/cssm_fleet.hip, fleet_create); the scan phases of
k_fleet_series give thread tid the particles tid * it .. tid * it + it - 1, it = ceil(N / threads) (csrc/cssm_fleet.hip.h), and every
sort of a row pads its N keys to np2, the power of two >= max(N, 2).  The lists the other fleet files run -- 1, 2, 63, 100, 257, 1000,
4096 -- leave out (tests/test_fleet_matrix_host.py asserts the arithmetic on a mirror of these formulas):

  N = 64    64 threads, it = 1: one full wave, nothing idle, np2 = N;
  N = 65    64 threads, it = 2: lanes 33 .. 63 of the only wave own nothing, lane 32 a single particle; np2 = 128;
  N = 2049  512 threads, it = 5: threads 410 .. 511 own nothing, so wave 7 is idle AS A WHOLE in wave_scan_u128, the max-scan carry and
            the lane-63 hand-offs -- the only kind of N at which a wave has nothing to hand on; np2 = 4096: 2047 pad keys, the most;
  N = 4095  512 threads, it = 8: the last thread is one particle short; one pad key.

The fleet is ragged_c2(6): C2 (d = 3) with parameters of its own per series, six series of 5 .. 26 records with their own time steps
and missing patterns.  One test per kind of launch and N; the comparison rules are those of each kind's own file, imported from there:
everything is == / assert_array_equal but the means, which keep the bounds their files state.  No series, row or N is skipped or
excused."""
import numpy as np
import pytest

from composablestatespacemodels_amd.filter import NativePfFleet
from test_forecast_draws import build_twin
from test_gpu_fleet import assert_series_equal_oracle, assert_summary_equal_oracle, ragged_c2
from test_gpu_fleet_filter import assert_filter_equals_oracle
from test_gpu_fleet_filter_forecasts import assert_whole_fleet_equals_the_loop, record_keys
from test_gpu_fleet_forecast import equal_bits, fc_key, held_to_the_oracle
from test_gpu_fleet_interpolate import assert_interpolation_equal, oracle_interpolate
from test_gpu_fleet_intervals import assert_whole_series_equals_the_oracle, oracle_rows
from test_gpu_fleet_step_interpolate import stream_and_check
from test_gpu_forecast import check_forecast, horizon_times

pytestmark = pytest.mark.gpu

EDGE_N = [64, 65, 2049, 4095]
S = 6
CSSM_OPT_FLEET_SELECT = 12                                     # include/cssm_pf.h: 1 the bitonic sort, 2 the radix select


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    return build_twin(tmp_path_factory.mktemp("twin"))


def fleet(n, count=1):
    """`count` fleets of ragged_c2(6)'s models and seeds at n particles, and the data"""
    models, seeds, datas = ragged_c2(S)
    fls = [NativePfFleet(models[0], n, S) for _ in range(count)]
    for f in fls:
        f.set_params(models); f.reseed(seeds)
    return fls, models, seeds, datas


# plain + k_fleet_summary ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", EDGE_N)
def test_ll_filter_and_summary(n):
    (fl,), models, seeds, datas = fleet(n)
    with fl:
        ll, ll_t, ess_t, rc = fl.ll_filter(datas)
        assert not rc.any(), rc
        orc = [assert_series_equal_oracle(fl, k, models[k], n, seeds[k], datas[k], ll, ll_t, ess_t) for k in range(S)]
        for interval in (0.975, 0.5):
            got = fl.summary(interval)
            for k in range(S):
                assert_summary_equal_oracle(got, k, orc[k], interval)


# PATH ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", EDGE_N)
def test_filter_paths(n):
    (fl,), models, seeds, datas = fleet(n)
    with fl:
        res = fl.filter(datas)
        assert not res[5].any(), res[5]
        for k in range(S):
            o = assert_filter_equals_oracle(res, k, models[k], n, seeds[k], datas[k])
            np.testing.assert_array_equal(fl.particles(k), o.particles())
            np.testing.assert_array_equal(fl.ancestors(k), o.ancestors())
            assert fl.observation_index(k) == len(datas[k][0])


# HIST + k_fleet_lineage ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", EDGE_N)
def test_interpolate_both_pairings(n):
    (fl,), models, seeds, datas = fleet(n)
    with fl:
        for pairing in (False, True):
            ll, rows, rc = fl.interpolate(datas, 0.975, pairing)
            assert not rc.any(), rc
            for k in range(S):
                assert rows[k][0].shape == (len(datas[k][0]) + 1, 3)
                assert_interpolation_equal(ll[k], rows[k], oracle_interpolate(models[k], n, seeds[k], datas[k], pairing))


# IVAL ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", EDGE_N)
def test_filter_intervals(n):
    (fl,), models, seeds, datas = fleet(n)
    intervals = (0.975, 1.0)
    with fl:
        want = [oracle_rows(models[k], n, seeds[k], datas[k], intervals) for k in range(S)]
        for iv in intervals:
            res = fl.filter_intervals(datas, iv)
            for k in range(S):
                assert_whole_series_equals_the_oracle(fl, k, res, want[k], iv, n, "exp", (n, iv, k))


# FCST ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", EDGE_N)
def test_filter_forecasts(n, twin):
    (fl, ref), models, seeds, datas = fleet(n, 2)
    with fl, ref:
        first_and_last = [(0, len(d[0]) - 1) for d in datas]
        assert_whole_fleet_equals_the_loop(fl, ref, models, datas, record_keys(datas), 0.975, first_and_last, twin)


# RING + k_fleet_window -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", EDGE_N)
def test_step_interpolate_stream(n):
    """the first 8 calls of the stream (series 0 ends after 5: inactive from then on), a window of 4 slices, lag 3 asked for throughout"""
    (fl,), models, seeds, datas = fleet(n)
    slices = 4
    with fl:
        fl.window(slices)
        fl.init([float(d[0][0]) for d in datas])
        stream_and_check(fl, models, seeds, datas, slices, lambda m: 3, 3, calls=8)
        assert [fl.window_depth(k) for k in range(S)] == [3] * S


# k_fleet_forecast ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", EDGE_N)
def test_forecast_by_sort_and_by_select(n, twin):
    (fl,), models, seeds, datas = fleet(n)
    clock = [float(d[0][-1]) for d in datas]
    times = [horizon_times(clock[k])[:1 + k % 3] for k in range(S)]       # 1 .. 3 horizons; equal times among them (a dt = 0 step)
    keys = [fc_key(k) for k in range(S)]
    with fl:
        _, _, _, rc = fl.ll_filter(datas)
        assert not rc.any(), rc
        fl.set_option(CSSM_OPT_FLEET_SELECT, 1)
        by_sort = fl.forecast(times, keys, 0.975, want_samples=True)
        exp = [held_to_the_oracle(fl, k, models[k], clock[k], times[k], by_sort[k], twin, 0.975) for k in range(S)]
        fl.set_option(CSSM_OPT_FLEET_SELECT, 2)
        by_select = fl.forecast(times, keys, 0.975, want_samples=True)
        for k in range(S):
            assert by_select[k]["rc"] == 0 and by_select[k]["key"] == keys[k]
            check_forecast(by_select[k], *exp[k], interval=0.975)
            equal_bits(by_select[k], by_sort[k])
