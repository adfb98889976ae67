"""CPU-only checks of the fleet's one-step-ahead forecasts (include/cssm_pf.h: cssm_fleet_filter_forecasts, cssm_fleet_step_forecast):
both symbols are exported with the header's signatures and bound, and what needs no fleet is refused -- with CSSM_EINVAL_ARG and a
message -- before the fleet is looked at, so on a host without a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from composablestatespacemodels_amd import _abi, load_library
from composablestatespacemodels_amd.filter import FilterFleet, NativePfFleet

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "cssm_pf.h")

_CTYPES = {"cssm_fleet*": C.c_void_p, "const uint64_t*": C.POINTER(C.c_uint64), "const double*": C.POINTER(C.c_double),
           "double*": C.POINTER(C.c_double), "const uint8_t*": C.POINTER(C.c_uint8), "int32_t*": C.POINTER(C.c_int32),
           "int*": C.POINTER(C.c_int), "double": C.c_double}

NAMES = ["cssm_fleet_filter_forecasts", "cssm_fleet_step_forecast"]


def _header_args(name):
    """the argument types of `int name(...)` as include/cssm_pf.h declares it"""
    src = open(HEADER).read()
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
    assert m, f"{name} is not declared in include/cssm_pf.h"
    out = []
    for a in m.group(1).split(","):
        ty = re.sub(r"\s+", " ", a.strip()).rsplit(" ", 1)[0]          # drop the parameter's name
        out.append(_CTYPES[ty])
    return out


@pytest.mark.parametrize("name", NAMES)
def test_exported_with_the_headers_signature_and_bound(name):
    lib = load_library()
    bound = {n: (res, args) for n, res, args in _abi.SYMBOLS}
    assert name in bound, f"{name} is not bound in _abi.SYMBOLS"
    res, args = bound[name]
    assert res is C.c_int
    assert args == _header_args(name)
    fn = getattr(lib, name)                                              # AttributeError if the library does not export it
    assert fn.restype is C.c_int and list(fn.argtypes) == args


def test_the_header_signatures_are_the_documented_ones():
    D, cD, I32, U8, U64, I = (C.POINTER(C.c_double),) * 2 + (C.POINTER(C.c_int32), C.POINTER(C.c_uint8), C.POINTER(C.c_uint64), C.POINTER(C.c_int))
    nine = [D] * 9
    assert _header_args("cssm_fleet_filter_forecasts") == [C.c_void_p, U64, cD, cD, U8, U64, C.c_double, D, D, I32] + nine + [I32, I32, I, I]
    assert _header_args("cssm_fleet_step_forecast") == [C.c_void_p, U8, cD, cD, U8, U64, C.c_double, D, I32] + nine + [I32, I32, I, I]


def _p(a, ty):
    return None if a is None else a.ctypes.data_as(C.POINTER(ty))


def _filter_forecasts(lib, fleet, off, t, y, interval, ll, rc, fc_rc):
    return lib.cssm_fleet_filter_forecasts(fleet, _p(off, C.c_uint64), _p(t, C.c_double), _p(y, C.c_double), None, None, interval,
                                           _p(ll, C.c_double), None, None, *([None] * 11), _p(rc, C.c_int), _p(fc_rc, C.c_int))


def test_filter_forecasts_refusals_need_no_fleet():
    """every refusal arrives although the fleet is null: it is made before the fleet is looked at"""
    lib = load_library()
    off = np.array([0, 2], dtype=np.uint64); t = np.zeros(2); y = np.zeros(2); ll = np.full(1, 7.0)
    rc = np.full(1, 7, dtype=np.int32); fc = np.full(1, 7, dtype=np.int32)
    bad_off = np.array([1, 2], dtype=np.uint64)
    ok = 0.975
    cases_ = [("off", (None, t, y, ok, ll, rc, fc)), ("ll_out", (off, t, y, ok, None, rc, fc)), ("rc_out", (off, t, y, ok, ll, None, fc)),
              ("fc_rc_out", (off, t, y, ok, ll, rc, None)), ("data", (off, None, y, ok, ll, rc, fc)), ("data", (off, t, None, ok, ll, rc, fc)),
              ("off[0]", (bad_off, t, y, ok, ll, rc, fc)), ("interval", (off, t, y, 0.0, ll, rc, fc)), ("interval", (off, t, y, -0.5, ll, rc, fc)),
              ("interval", (off, t, y, 1.0000001, ll, rc, fc)), ("interval", (off, t, y, float("nan"), ll, rc, fc)),
              ("fleet", (off, t, y, ok, ll, rc, fc)), ("fleet", (off, t, y, 1.0, ll, rc, fc))]
    for word, a in cases_:
        assert _filter_forecasts(lib, None, *a) == _abi.CSSM_EINVAL_ARG, word
        msg = lib.cssm_last_error().decode()
        assert word in msg, (word, msg)
    assert list(ll) == [7.0] and list(rc) == [7] and list(fc) == [7]     # nothing was written


def test_step_forecast_refusals_need_no_fleet():
    lib = load_library()
    t = np.zeros(2); rc = np.full(2, 7, dtype=np.int32); fc = np.full(2, 7, dtype=np.int32)
    call = lambda tt, yy, interval, r, q: lib.cssm_fleet_step_forecast(None, None, _p(tt, C.c_double), _p(yy, C.c_double), None, None, interval,
                                                                       None, None, *([None] * 11), _p(r, C.c_int), _p(q, C.c_int))
    for word, a in [("null", (None, t, 0.975, rc, fc)), ("null", (t, None, 0.975, rc, fc)), ("null", (t, t, 0.975, None, fc)),
                    ("null", (t, t, 0.975, rc, None)), ("interval", (t, t, 0.0, rc, fc)), ("interval", (t, t, 1.5, rc, fc)),
                    ("interval", (t, t, float("nan"), rc, fc)), ("fleet", (t, t, 0.975, rc, fc)), ("fleet", (t, t, 1.0, rc, fc))]:
        assert call(*a) == _abi.CSSM_EINVAL_ARG, word
        msg = lib.cssm_last_error().decode()
        assert word in msg, (word, msg)
    assert list(rc) == [7, 7] and list(fc) == [7, 7]


def test_python_surface_rejects_a_wrong_number_of_series_or_keys_before_any_device_call():
    fl = NativePfFleet.__new__(NativePfFleet)
    fl.S, fl.n, fl.d, fl.generation, fl._h, fl.lib, fl.seeds = 3, 10, 1, 0, C.c_void_p(), None, [0] * 3
    three = [(np.zeros(2), np.zeros(2), None)] * 3
    with pytest.raises(ValueError, match="per series"):
        fl.filter_forecasts(three[:2])
    with pytest.raises(ValueError, match="keys per series"):
        fl.filter_forecasts(three, keys=[[1, 2]] * 2)
    with pytest.raises(ValueError, match="one key per record"):
        fl.filter_forecasts(three, keys=[[1, 2], [1, 2, 3], [1, 2]])
    with pytest.raises(ValueError, match="per series"):
        fl.step_forecast(np.zeros(2), np.zeros(2))
    with pytest.raises(ValueError, match="key per series"):
        fl.step_forecast(np.zeros(3), np.zeros(3), keys=[1, 2])
    assert fl.generation == 0                                            # nothing was started
    ff = FilterFleet.__new__(FilterFleet)
    ff._fleet, ff.S = fl, 3
    with pytest.raises(ValueError, match="per series"):
        ff.stepForecast([], [None] * 3)
    with pytest.raises(ValueError, match="per series"):
        ff.filterForecasts([[]] * 2)
