"""CPU-only checks of the fleet interpolation's host side (include/cssm_pf.h: cssm_fleet_interpolate, cssm_fleet_interpolate_last_ms):
the exported symbols, the refusals that are made before the fleet is looked at, the ragged unpacking of NativePfFleet.interpolate and
the one PfOut construction FilterInterpolate and FilterFleet share."""
import ctypes as C

import numpy as np
import pytest

import cases
from composablestatespacemodels_amd import Data, _abi, load_library
from composablestatespacemodels_amd import filter as flt
from composablestatespacemodels_amd.filter import FilterFleet, FilterInterpolate, NativePfFleet, PfOut


def _handleless(S=3, n=10, d=1):
    """a fleet object without a handle: whatever it refuses, it refuses before any device call"""
    fl = NativePfFleet.__new__(NativePfFleet)
    fl.S, fl.n, fl.d, fl.generation, fl._h, fl.lib, fl.seeds = S, n, d, 0, C.c_void_p(), None, [0] * S
    return fl


def _p(a, ty):
    return a.ctypes.data_as(C.POINTER(ty))


def test_the_library_exports_the_entry_points_with_the_abi_signatures():
    lib = load_library()
    sig = {name: (res, args) for name, res, args in _abi.SYMBOLS}
    u64p, dp, u8p = C.POINTER(C.c_uint64), C.POINTER(C.c_double), C.POINTER(C.c_uint8)
    assert sig["cssm_fleet_interpolate"] == (C.c_int, [C.c_void_p, u64p, dp, dp, u8p, C.c_double, C.c_int] + [dp] * 7 + [C.POINTER(C.c_int)])
    assert sig["cssm_fleet_interpolate_last_ms"] == (C.c_int, [C.c_void_p, dp])
    for name in ("cssm_fleet_interpolate", "cssm_fleet_interpolate_last_ms"):
        fn = getattr(lib, name)                                # AttributeError if libcssm_pf.so does not export it
        assert fn.restype is sig[name][0] and list(fn.argtypes) == sig[name][1]
    assert _abi.CSSM_OPT_INTERP_CAP == 13
    assert _abi.CSSM_INTERP_REFERENCE_PAIRING == 1


def _call(lib, f=None, off=(0, 2), interval=0.975, flags=0, null_off=False):
    off = np.asarray(off, dtype=np.uint64)
    t = np.arange(4.0); y = np.ones(4); ll = np.zeros(1); rc = np.zeros(1, dtype=np.int32)
    return lib.cssm_fleet_interpolate(f, None if null_off else _p(off, C.c_uint64), _p(t, C.c_double), _p(y, C.c_double), None, interval, flags,
                                      _p(ll, C.c_double), *([None] * 6), _p(rc, C.c_int))


def test_whole_call_refusals_are_made_before_the_fleet_is_looked_at():
    lib = load_library()
    for kw, word in (({}, b"null fleet"), ({"null_off": True}, b"off is null"), ({"off": (1, 2)}, b"off[0] must be 0"),
                     ({"interval": 1.5}, b"interval must be in (0, 1]"), ({"flags": 6}, b"unknown flag bits 0x6")):
        assert _call(lib, **kw) == _abi.CSSM_EINVAL_ARG, kw
        assert word in lib.cssm_last_error(), (kw, lib.cssm_last_error())
    off = np.zeros(2, dtype=np.uint64); t = np.zeros(1); rc = np.zeros(1, dtype=np.int32); ll = np.zeros(1)
    assert lib.cssm_fleet_interpolate(None, _p(off, C.c_uint64), _p(t, C.c_double), _p(t, C.c_double), None, 0.975, 0, None, *([None] * 6),
                                      _p(rc, C.c_int)) == _abi.CSSM_EINVAL_ARG
    assert b"ll_out / rc_out is null" in lib.cssm_last_error()
    assert lib.cssm_fleet_interpolate(None, _p(off, C.c_uint64), None, _p(t, C.c_double), None, 0.975, 0, _p(ll, C.c_double), *([None] * 6),
                                      _p(rc, C.c_int)) == _abi.CSSM_EINVAL_ARG
    assert b"null data" in lib.cssm_last_error()


def test_last_ms_without_a_fleet_leaves_the_array_alone():
    lib = load_library()
    ms = np.full(2, 7.0)
    assert lib.cssm_fleet_interpolate_last_ms(None, _p(ms, C.c_double)) == _abi.CSSM_EINVAL_ARG and list(ms) == [7.0, 7.0]
    assert b"null" in lib.cssm_last_error()


def test_a_wrong_number_of_series_is_rejected_before_any_device_call():
    fl = _handleless(3)
    one = (np.arange(2.0), np.ones(2), None)
    with pytest.raises(ValueError, match="per series"):
        fl.interpolate([one, one])
    with pytest.raises(ValueError, match="per series"):
        fl.interpolate([one] * 4, reference_pairing=True)
    off, t, y, has = NativePfFleet.pack([one, one])
    with pytest.raises(ValueError, match="S \\+ 1 = 4"):
        fl.interpolate_packed(off, t, y, has)
    ff = FilterFleet.__new__(FilterFleet)
    ff._fleet, ff.S = fl, 3
    with pytest.raises(ValueError, match="per series"):
        ff.interpolate([[Data(0.0, 1.0)]])


def test_row_offsets_of_a_ragged_list_with_an_empty_and_a_one_record_series():
    datas = [(np.arange(3.0), np.ones(3), None), (np.zeros(0), np.zeros(0), None), (np.array([5.0]), np.array([2.0]), np.array([0])),
             (np.arange(4.0), np.ones(4))]
    with pytest.raises(ValueError, match="series 1 has no records"):
        NativePfFleet.pack(datas)                              # (the filters still refuse it)
    off, t, y, has = NativePfFleet.pack(datas, allow_empty=True)
    assert off.dtype == np.uint64 and list(off) == [0, 3, 3, 4, 8]
    assert list(t) == [0, 1, 2, 5, 0, 1, 2, 3] and list(has) == [1, 1, 1, 0, 1, 1, 1, 1] and has.dtype == np.uint8
    rows, d = int(off[-1]) + 4, 2
    m = np.arange(rows * d, dtype=np.float64).reshape(rows, d)
    e = np.arange(rows, dtype=np.float64)
    per = NativePfFleet.interpolate_rows(off, (m, m + 0.25, m + 0.5, e, e + 0.25, e + 0.5))
    assert len(per) == 4
    first = [0, 4, 5, 7]                                       # off[k] + k
    for k, T in enumerate((3, 0, 1, 4)):
        assert len(per[k]) == 6
        assert per[k][0].shape == (T + 1, d) and per[k][3].shape == (T + 1,)
        np.testing.assert_array_equal(per[k][0], m[first[k]:first[k] + T + 1])
        np.testing.assert_array_equal(per[k][2], m[first[k]:first[k] + T + 1] + 0.5)
        np.testing.assert_array_equal(per[k][4], e[first[k]:first[k] + T + 1] + 0.25)
    assert first[3] + 4 + 1 == rows                            # the last series ends the arrays


@pytest.mark.parametrize("pairing", [False, True])
def test_one_pfout_construction_for_both_filters(pairing, monkeypatch):
    """FilterInterpolate.interpolate and FilterFleet.interpolate hand the arrays of one series to the same helper and return the same
    objects: observation None at row 0 and at gap rows, the times in the order given behind the smallest one."""
    data = [Data(3.0, 1.0), Data(4.0, None), Data(5.0, None), Data(6.0, 4.0), Data(2.5, 0.0)]
    T, d = len(data), 3
    rng = np.random.default_rng(7)
    arrays = (rng.normal(size=(T + 1, d)), rng.normal(size=(T + 1, d)), rng.normal(size=(T + 1, d)), rng.normal(size=T + 1),
              rng.normal(size=T + 1), rng.normal(size=T + 1))
    seen = []

    class OneHandle:
        n = 50

        def interpolate(self, t, y, h, interval, reference_pairing):
            seen.append(("single", list(t), list(y), list(h), interval, reference_pairing))
            return (-12.5,) + arrays

    class Fleet:
        def interpolate(self, split, interval, reference_pairing):
            seen.append(("fleet", [list(s[0]) for s in split], interval, reference_pairing))
            return np.array([-12.5, -1.0]), [arrays, tuple(a[:2] for a in arrays)], np.zeros(2, dtype=np.int32)

    fi = FilterInterpolate.__new__(FilterInterpolate)
    fi._pf = OneHandle()
    monkeypatch.setattr(FilterInterpolate, "_ensure", lambda self, n: self._pf)
    ll1, out1 = fi.interpolate(data, 50, 0.9, pairing)
    ff = FilterFleet.__new__(FilterFleet)
    ff._fleet, ff.S = Fleet(), 2
    (ll2, out2), (ll3, out3) = ff.interpolate([data, data[:1]], 0.9, pairing)
    assert seen[0][4:] == (0.9, pairing) and seen[1][2:] == (0.9, pairing)
    assert ll1 == ll2 == -12.5 and ll3 == -1.0 and len(out1) == len(out2) == T + 1 and len(out3) == 2
    assert [o.time for o in out1] == [2.5, 3.0, 4.0, 5.0, 6.0, 2.5]
    assert [o.observation for o in out1] == [None, 1.0, None, None, 4.0, 0.0]
    for a, b in zip(out1, out2):
        assert isinstance(a, PfOut) and isinstance(b, PfOut)
        assert (a.time, a.observation, a.eta, a.etaIntervals, a.stateIntervals) == (b.time, b.observation, b.eta, b.etaIntervals, b.stateIntervals)
        np.testing.assert_array_equal(a.state, b.state)
    for k, o in enumerate(out1):
        assert o.eta == arrays[3][k] and (o.etaIntervals.lower, o.etaIntervals.upper) == (arrays[4][k], arrays[5][k])
        np.testing.assert_array_equal(o.state, arrays[0][k])
        assert [(c.lower, c.upper) for c in o.stateIntervals] == list(zip(arrays[1][k], arrays[2][k]))
    assert [o.time for o in out3] == [3.0, 3.0] and [o.observation for o in out3] == [None, 1.0]
    # the helper itself, called directly, is what both went through
    direct = flt._interpolate_outs(data, np.array([x.t for x in data]), arrays)
    assert [(o.time, o.observation, o.eta) for o in direct] == [(o.time, o.observation, o.eta) for o in out1]


def test_a_series_with_a_status_raises_naming_the_series():
    from composablestatespacemodels_amd import CssmError

    class Fleet:
        def interpolate(self, split, interval, reference_pairing):
            a = tuple(np.full((2, 1), np.nan) for _ in range(3)) + tuple(np.full(2, np.nan) for _ in range(3))
            return np.array([0.0, np.nan]), [a, a], np.array([0, _abi.CSSM_ENONFINITE], dtype=np.int32)

    ff = FilterFleet.__new__(FilterFleet)
    ff._fleet, ff.S = Fleet(), 2
    with pytest.raises(CssmError, match="series 1") as e:
        ff.interpolate([[Data(0.0, 1.0)], [Data(0.0, 1.0)]])
    assert e.value.code == _abi.CSSM_ENONFINITE
