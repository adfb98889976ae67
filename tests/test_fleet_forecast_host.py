"""CPU-only checks of the fleet forecast's host side (include/cssm_pf.h: cssm_fleet_forecast, cssm_fleet_observation_index): the
ragged packing of NativePfFleet.forecast, refusals that need no device, and the entry points' behaviour without a fleet."""
import ctypes as C
import os

import numpy as np
import pytest

import cases
from composablestatespacemodels_amd import _abi, load_library
from composablestatespacemodels_amd.filter import FilterFleet, NativePfFleet


def _handleless(S=3, n=10, d=1):
    """a fleet object without a handle: whatever it refuses, it refuses before any device call"""
    fl = NativePfFleet.__new__(NativePfFleet)
    fl.S, fl.n, fl.d, fl.generation, fl._h, fl.lib, fl.seeds = S, n, d, 0, C.c_void_p(), None, [0] * S
    return fl


def test_ragged_times_packing():
    fl = _handleless(5)
    off, t = fl.pack_times([np.arange(3.0), None, np.array([5, 4], dtype=np.int64), np.zeros(0), np.arange(10.0, dtype=np.float32)[::5]])
    assert off.dtype == np.uint64 and list(off) == [0, 3, 3, 5, 5, 7]
    assert t.dtype == np.float64 and t.flags.c_contiguous and list(t) == [0, 1, 2, 5, 4, 0, 5]
    off, t = fl.pack_times([None, [], (), np.zeros(0), None])
    assert off.dtype == np.uint64 and list(off) == [0] * 6 and t.dtype == np.float64 and len(t) == 0
    off, t = fl.pack_times([[1.5]] * 5)
    assert list(off) == [0, 1, 2, 3, 4, 5] and list(t) == [1.5] * 5


def test_a_wrong_number_of_series_is_rejected_before_any_device_call():
    fl = _handleless(3)
    with pytest.raises(ValueError, match="per series"):
        fl.forecast([[1.0], [2.0]])
    with pytest.raises(ValueError, match="per series"):
        fl.forecast([[1.0]] * 4, keys=[1, 2, 3, 4])
    with pytest.raises(ValueError, match="one key per series"):
        fl.forecast([[1.0]] * 3, keys=[1, 2])
    ff = FilterFleet.__new__(FilterFleet)
    ff._fleet, ff.S = fl, 3
    with pytest.raises(ValueError, match="per series"):
        ff.forecast([[1.0]])


def test_entry_points_without_a_fleet():
    lib = load_library()
    assert lib.cssm_fleet_observation_index(None, 0) == 0 and lib.cssm_fleet_observation_index(None, 7) == 0
    off = np.zeros(2, dtype=np.uint64); t = np.zeros(1); ky = np.zeros(1, dtype=np.uint64); rc = np.zeros(1, dtype=np.int32)
    p = lambda a, ty: a.ctypes.data_as(C.POINTER(ty))
    assert lib.cssm_fleet_forecast(None, p(off, C.c_uint64), p(t, C.c_double), p(ky, C.c_uint64), 0.975, *([None] * 10),
                                   p(rc, C.c_int)) == _abi.CSSM_EINVAL_ARG
    assert b"null" in lib.cssm_last_error()
    ms = np.full(3, 7.0)
    assert lib.cssm_fleet_last_ms(None, p(ms, C.c_double)) == _abi.CSSM_EINVAL_ARG and list(ms) == [7.0] * 3
    if not os.path.exists("/dev/kfd"):   # without a device the forecast is never reached: no fleet comes into being
        h = C.c_void_p()
        assert lib.cssm_fleet_create(cases.c2_model().descriptor().ptr(), 100, 4, 0, C.byref(h)) == _abi.CSSM_EHIP and not h.value
