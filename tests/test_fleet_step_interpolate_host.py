"""CPU-only checks of the fleet's streaming interpolation (include/cssm_pf.h: cssm_fleet_window, cssm_fleet_window_depth,
cssm_fleet_step_interpolate, cssm_fleet_step_interpolate_last_ms): the refusals that precede any look at the fleet -- shown on a null
fleet, each with its message --, the Python argument checks that need no handle, and the constants of the ctypes view."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from composablestatespacemodels_amd import _abi, load_library
from composablestatespacemodels_amd.filter import NativePfFleet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_dp, _u32p, _ip = C.POINTER(C.c_double), C.POINTER(C.c_uint32), C.POINTER(C.c_int)


def _call(lib, t=True, y=True, rc=True, lag=None, max_lag=0, interval=0.975, fleet=None):
    """cssm_fleet_step_interpolate on `fleet` (null) with one series' worth of arguments; the missing ones null"""
    tt, yy, rr = (C.c_double * 1)(1.0), (C.c_double * 1)(2.0), (C.c_int * 1)(0)
    lg = None if lag is None else (C.c_uint32 * len(lag))(*lag)
    return lib.cssm_fleet_step_interpolate(fleet, None, tt if t else None, yy if y else None, None, lg, max_lag, interval, None, None, None,
                                           None, None, None, None, None, None, rr if rc else None)


def test_refusals_come_before_the_fleet_is_looked_at():
    lib = load_library()
    for kw, word in (({"t": False}, b"null argument"), ({"y": False}, b"null argument"), ({"rc": False}, b"null argument"),
                     ({"interval": 0.0}, b"interval must be in (0, 1]"), ({"interval": 1.5}, b"interval must be in (0, 1]"),
                     ({"interval": float("nan")}, b"interval must be in (0, 1]"),
                     ({"lag": [4], "max_lag": 3}, b"lag[0] = 4 is above max_lag = 3"),
                     ({"max_lag": _abi.CSSM_FLEET_NO_ROWS}, b"CSSM_FLEET_NO_ROWS"),
                     ({}, b"null fleet"), ({"lag": [3], "max_lag": 3}, b"null fleet"),
                     ({"lag": [_abi.CSSM_FLEET_NO_ROWS], "max_lag": 0}, b"null fleet")):       # (no rows is no bad lag)
        assert _call(lib, **kw) == _abi.CSSM_EINVAL_ARG, kw
        assert word in lib.cssm_last_error(), (kw, lib.cssm_last_error())


def test_window_calls_on_a_null_fleet():
    lib = load_library()
    assert lib.cssm_fleet_window(None, 1) == _abi.CSSM_EINVAL_ARG                              # refused whatever the fleet
    assert b"at least 2" in lib.cssm_last_error()
    for slices in (0, 2, 16):
        assert lib.cssm_fleet_window(None, slices) == _abi.CSSM_EINVAL_ARG
        assert b"null fleet" in lib.cssm_last_error()
    assert lib.cssm_fleet_window_depth(None, 0) == 0 and lib.cssm_fleet_window_depth(None, 7) == 0
    ms = (C.c_double * 2)()
    assert lib.cssm_fleet_step_interpolate_last_ms(None, ms) == _abi.CSSM_EINVAL_ARG


def _handleless(S=3, d=2):
    fl = NativePfFleet.__new__(NativePfFleet)
    fl.S, fl.n, fl.d, fl.generation, fl._h, fl.lib = S, 10, d, 0, C.c_void_p(), None
    return fl


def test_python_argument_checks_need_no_handle():
    fl = _handleless()
    z = np.zeros(3)
    with pytest.raises(ValueError, match="one lag per series"):
        fl.step_interpolate(z, z, lag=[1, 2], max_lag=2)
    with pytest.raises(ValueError, match="max_lag"):
        fl.step_interpolate(z, z, max_lag=-1)
    with pytest.raises(ValueError, match="negative"):
        fl.step_interpolate(z, z, lag=[0, -1, 0], max_lag=2)
    with pytest.raises(ValueError, match=r"one \(t, y\) per series"):
        fl.step_interpolate(np.zeros(2), z, max_lag=1)
    with pytest.raises(ValueError, match="negative"):
        fl.window(-1)
    lg = fl._lags([2, None, 0], 2)
    assert lg.dtype == np.uint32 and list(lg) == [2, _abi.CSSM_FLEET_NO_ROWS, 0]
    assert list(fl._lags(1, 3)) == [1, 1, 1] and fl._lags(None, 3) is None


def test_abi_constants_equal_the_header():
    src = open(os.path.join(ROOT, "include", "cssm_pf.h")).read()
    assert _abi.CSSM_FLEET_NO_ROWS == int(re.search(r"#define CSSM_FLEET_NO_ROWS (0x[0-9a-fA-F]+)u", src).group(1), 16) == 2**32 - 1
    bound = {s[0]: s for s in _abi.SYMBOLS}
    lib = load_library()
    for name in ("cssm_fleet_window", "cssm_fleet_window_depth", "cssm_fleet_step_interpolate", "cssm_fleet_step_interpolate_last_ms"):
        assert name in bound and hasattr(lib, name)
    assert bound["cssm_fleet_window_depth"][1] is C.c_uint32
    assert len(bound["cssm_fleet_step_interpolate"][2]) == 18
