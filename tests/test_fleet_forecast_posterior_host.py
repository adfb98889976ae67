"""CPU-only checks of the fleet posterior forecast's host side (include/cssm_pf.h: cssm_fleet_forecast_posterior): the ragged packing of
NativePfFleet.pack_posteriors, refusals that need no device, the per-chain rows of a fleet PMMH, and the entry point without a fleet."""
import ctypes as C

import numpy as np
import pytest

import cases
from composablestatespacemodels_amd import _abi, load_library
from composablestatespacemodels_amd.filter import FilterFleet
from composablestatespacemodels_amd.pmmh import fleet_posterior_rows, posterior_rows
from test_fleet_forecast_host import _handleless


def test_ragged_posteriors_packing():
    fl = _handleless(5, d=2)
    rng = np.random.default_rng(1)
    th = [rng.standard_normal((m, 3)) for m in (2, 0, 1, 0, 4)]
    xs = [rng.standard_normal((m, 2)) for m in (2, 0, 1, 0, 4)]
    # a Fortran-ordered block, float32 rows, None and empty arrays for M_k = 0, one row given flat
    post = [(np.asfortranarray(th[0]), xs[0]), None, (th[2][0].astype(np.float32), xs[2][0]), (np.zeros((0, 3)), np.zeros((0, 2))), (th[4], xs[4].ravel())]
    moff, theta, x = fl.pack_posteriors(post)
    assert moff.dtype == np.uint64 and list(moff) == [0, 2, 2, 3, 3, 7]
    assert theta.dtype == np.float64 and theta.flags.c_contiguous and theta.shape == (7, 3)
    assert x.dtype == np.float64 and x.flags.c_contiguous and x.shape == (7, 2)
    np.testing.assert_array_equal(theta[:2], th[0]); np.testing.assert_array_equal(x[:2], xs[0])
    np.testing.assert_array_equal(theta[2], th[2][0].astype(np.float32)); np.testing.assert_array_equal(x[2], xs[2][0])
    np.testing.assert_array_equal(theta[3:], th[4]); np.testing.assert_array_equal(x[3:], xs[4])
    moff, theta, x = fl.pack_posteriors([None] * 5, n_theta=6)      # nobody has a row: the caller (or the fleet's descriptor) names its length
    assert list(moff) == [0] * 6 and theta.shape == (0, 6) and x.shape == (0, 2) and theta.flags.c_contiguous and x.flags.c_contiguous
    fl.n_theta = 3                                                  # what a fleet with a descriptor knows
    assert fl.pack_posteriors([None] * 5)[1].shape == (0, 3)
    with pytest.raises(ValueError, match="series 0"):
        fl.pack_posteriors([(th[0][:, :2], xs[0]), None, None, None, None])                    # rows that are not the descriptor's
    del fl.n_theta
    with pytest.raises(ValueError, match="series 4"):
        fl.pack_posteriors([(th[0], xs[0]), None, None, None, (th[4][:, :2], xs[4])])          # rows of another length
    with pytest.raises(ValueError, match="series 0"):
        fl.pack_posteriors([(th[0], np.zeros((2, 3))), None, None, None, None])                # states of another dimension


def test_a_wrong_number_of_series_keys_or_t0s_is_rejected_before_any_device_call():
    fl = _handleless(3, n=10, d=1)
    post = [(np.zeros((2, 4)), np.zeros((2, 1)))] * 3
    times = [[1.0]] * 3
    with pytest.raises(ValueError, match="per series"):
        fl.forecast_posterior(post[:2], 0.0, times, keys=[1, 2, 3])
    with pytest.raises(ValueError, match="per series"):
        fl.forecast_posterior(post, 0.0, times[:2], keys=[1, 2, 3])
    with pytest.raises(ValueError, match="one t0 per series"):
        fl.forecast_posterior(post, [0.0, 1.0], times, keys=[1, 2, 3])
    with pytest.raises(ValueError, match="one key per series"):
        fl.forecast_posterior(post, 0.0, times, keys=[1, 2])
    with pytest.raises(ValueError, match="picks"):
        fl.forecast_posterior(post, 0.0, times, keys=[1, 2, 3], picks=np.zeros((3, 9), dtype=np.int64))
    with pytest.raises(ValueError, match="picks"):
        fl.forecast_posterior(post, 0.0, times, keys=[1, 2, 3], picks=-np.ones((3, 10), dtype=np.int64))


def test_filter_fleet_argument_checks():
    ff = FilterFleet.__new__(FilterFleet)
    ff._fleet, ff.S = _handleless(2, n=10, d=1), 2
    arrays = (np.zeros((2, 4)), np.zeros((2, 1)))
    with pytest.raises(ValueError, match="per series"):
        ff.forecastPosterior([arrays], 0.0, [[1.0], [1.0]], params=object())
    with pytest.raises(ValueError, match="per series"):
        ff.forecastPosterior([arrays, arrays], 0.0, [[1.0]], params=object())
    with pytest.raises(ValueError, match="one t0 per series"):
        ff.forecastPosterior([arrays, arrays], [0.0, 1.0, 2.0], [[1.0], [1.0]], params=object())
    with pytest.raises(ValueError, match="params"):
        ff.forecastPosterior([arrays, arrays], 0.0, [[1.0], [1.0]])                             # arrays without the tree they flatten
    with pytest.raises(ValueError, match="empty"):
        ff.forecastPosterior([[], []], 0.0, [[1.0], [1.0]])                                     # MetropStates: none


def test_per_chain_rows_of_a_fleet_pmmh():
    rng = np.random.default_rng(2)
    theta, last = rng.standard_normal((3, 12, 5)), rng.standard_normal((3, 12, 2))
    rows = fleet_posterior_rows(theta, last, burn_in=2, thin=2)
    assert len(rows) == 3
    for k, (th, xs) in enumerate(rows):
        a, b = posterior_rows(theta[k], last[k], 2, 2)
        assert th.shape == (5, 5) and xs.shape == (5, 2)
        np.testing.assert_array_equal(th, a); np.testing.assert_array_equal(xs, b)
        np.testing.assert_array_equal(th, theta[k, 2::2]); np.testing.assert_array_equal(xs, last[k, 2::2])
    with pytest.raises(ValueError):
        fleet_posterior_rows(theta[0], last[0])
    with pytest.raises(ValueError):
        fleet_posterior_rows(theta, last[:2])


def test_entry_point_without_a_fleet():
    lib = load_library()
    p = lambda a, ty: a.ctypes.data_as(C.POINTER(ty))
    desc = cases.c2_model().descriptor()
    u = np.zeros(2, dtype=np.uint64); dbl = np.zeros(8); ky = np.zeros(1, dtype=np.uint64); rc = np.full(1, 7, dtype=np.int32)
    args = (p(u, C.c_uint64), p(dbl, C.c_double), 1, p(dbl, C.c_double), p(dbl, C.c_double), p(u, C.c_uint64), p(dbl, C.c_double), None,
            p(ky, C.c_uint64), 0.975, *([None] * 11), p(rc, C.c_int))
    assert lib.cssm_fleet_forecast_posterior(None, desc.ptr(), *args) == _abi.CSSM_EINVAL_ARG
    assert b"null" in lib.cssm_last_error() and rc[0] == 7
