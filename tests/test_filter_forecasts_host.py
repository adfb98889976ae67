"""CPU-only checks of the single handle's one-step-ahead forecasts (include/cssm_pf.h: cssm_pf_filter_forecasts,
cssm_pf_filter_forecasts_more, cssm_pf_step_forecast, cssm_pf_forecasts_last_ms):

  * the bindings against the header, the refusals made before the GPU is looked at, the Python and C++ surfaces, and the default-key
    rule of the wrappers;
  * the premise the device rows rest on: the sequential twin of the two-rank selection (tests/cpp/intervals_twin.c), with the ranks
    the observation row takes (getOrderStatistic's, as eta), equals a sort of the order keys on the rows an observation draw produces
    -- counts with a handful of distinct values, 0/1 rows, one value only --, which are the selection's worst case (its picked
    sub-range holds most of the row) and here the ordinary one."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import cases
from composablestatespacemodels_amd import Data, _abi, load_library
from composablestatespacemodels_amd.filter import FORECAST_NAMES, Filter, FilterInit, ForecastOut, NativePf, Resampling
from test_filter_intervals_host import INTERVALS, SIZES, _bits, exact_order_statistics, twin_constants, twin_select

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_dp, _u64p, _i32p, _u8p = C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
NAMES = ("cssm_pf_filter_forecasts", "cssm_pf_filter_forecasts_more", "cssm_pf_step_forecast", "cssm_pf_forecasts_last_ms")
_H = C.c_void_p
BATCH = [_H, _dp, _dp, _u8p, C.c_size_t, _u64p, C.c_double, _dp, _dp, _i32p] + [_dp] * 9 + [_i32p, _i32p]
STEP = [_H, C.c_double, C.c_double, C.c_int, C.c_uint64, C.c_int, C.c_double, _dp, _i32p] + [_dp] * 9 + [_i32p, _i32p]


def test_the_four_symbols_with_the_declared_prototypes():
    lib = load_library()
    bound = {s[0]: s for s in _abi.SYMBOLS}
    for name in NAMES:
        assert name in bound and hasattr(lib, name), name
        assert bound[name][1] is C.c_int
    assert bound["cssm_pf_filter_forecasts"][2] == BATCH and bound["cssm_pf_filter_forecasts_more"][2] == BATCH
    assert bound["cssm_pf_step_forecast"][2] == STEP
    assert bound["cssm_pf_forecasts_last_ms"][2] == [_H, _dp]
    # ... and the header declares them with as many parameters
    hdr = open(os.path.join(ROOT, "include", "cssm_pf.h")).read()
    for name in NAMES:
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", hdr)
        assert m, name
        assert len(m.group(1).split(",")) == len(bound[name][2]), name


def test_refusals_through_the_bare_library():
    lib = load_library()
    A = _abi.CSSM_EINVAL_ARG
    t = np.zeros(2); tp = t.ctypes.data_as(_dp)
    outs = [None] * 11
    for fn in (lib.cssm_pf_filter_forecasts, lib.cssm_pf_filter_forecasts_more):
        assert fn(None, tp, tp, None, 2, None, 0.975, None, None, None, *outs) == A and b"null argument" in lib.cssm_last_error()
        assert fn(None, None, tp, None, 2, None, 0.975, None, None, None, *outs) == A
        assert fn(None, tp, None, None, 2, None, 0.975, None, None, None, *outs) == A
        assert fn(None, tp, tp, None, 0, None, 0.975, None, None, None, *outs) == A
        for bad in (0.0, 1.5, float("nan")):
            assert fn(None, tp, tp, None, 2, None, bad, None, None, None, *outs) == A
    assert lib.cssm_pf_step_forecast(None, 0.0, 0.0, 1, 0, 0, 0.975, None, None, *outs) == A and b"null handle" in lib.cssm_last_error()
    assert lib.cssm_pf_step_forecast(None, 0.0, 0.0, 1, 0, 0, 1.5, None, None, *outs) == A
    ms = np.full(2, 7.0)
    assert lib.cssm_pf_forecasts_last_ms(None, ms.ctypes.data_as(_dp)) == A and list(ms) == [7.0, 7.0]


# ---- the Python surface against a recording stub -------------------------------------------------------------------------------------
D_STUB, N_STUB, SEED_STUB, INDEX_STUB = 3, 11, 987654321, 5


class StubLib:
    """``NativePf.lib``: the calls check their argument count against ``_abi.SYMBOLS``, record their inputs and fill output j with
    1000 (j + 1) + index through the pointers they were given."""

    def __init__(self):
        self.calls = []
        self.sig = {s[0]: s[2] for s in _abi.SYMBOLS}
        self.real = load_library()

    def cssm_pf_run_key(self, seed, run):
        return self.real.cssm_pf_run_key(seed, run)

    def cssm_pf_observation_index(self, h):
        return INDEX_STUB

    def _rows(self, T, outs):
        assert len(outs) == 11
        for j, p in enumerate(outs):
            if p is not None:
                count = T * D_STUB if j < 3 else T
                a = np.ctypeslib.as_array(p, shape=(count,))
                a[:] = (1000 * (j + 1) + np.arange(count)).astype(a.dtype)

    def _batch(self, name, h, t, y, has, T, keys, interval, ll, ll_t, ess_t, *outs):
        assert 10 + len(outs) == len(self.sig[name])
        self.calls.append({"name": name, "T": T, "interval": interval, "t": np.ctypeslib.as_array(t, shape=(T,)).copy(),
                           "y": np.ctypeslib.as_array(y, shape=(T,)).copy(), "has": None if has is None else np.ctypeslib.as_array(has, shape=(T,)).copy(),
                           "keys": None if keys is None else np.ctypeslib.as_array(keys, shape=(T,)).copy()})
        ll._obj.value = 42.5
        np.ctypeslib.as_array(ll_t, shape=(T,))[:] = 10.0 + np.arange(T)
        np.ctypeslib.as_array(ess_t, shape=(T,))[:] = 20 + np.arange(T)
        self._rows(T, outs)
        return 0

    def cssm_pf_filter_forecasts(self, *a):
        return self._batch("cssm_pf_filter_forecasts", *a)

    def cssm_pf_filter_forecasts_more(self, *a):
        return self._batch("cssm_pf_filter_forecasts_more", *a)

    def cssm_pf_step_forecast(self, h, t, y, has, key, use_key, interval, ll, ess, *outs):
        assert 9 + len(outs) == len(self.sig["cssm_pf_step_forecast"])
        self.calls.append({"name": "cssm_pf_step_forecast", "t": t, "y": y, "has": has, "key": key, "use_key": use_key, "interval": interval})
        ll._obj.value, ess._obj.value = -3.5, 9
        self._rows(1, outs)
        return 0

    def cssm_pf_forecasts_last_ms(self, h, ms):
        np.ctypeslib.as_array(ms, shape=(2,))[:] = (3.0, 2.0)
        return 0

    def cssm_pf_init_from(self, h, t0, state):
        self.calls.append({"name": "cssm_pf_init_from", "t0": t0})
        return 0


def stub_pf() -> NativePf:
    pf = object.__new__(NativePf)
    pf.lib, pf._h, pf.n, pf.d, pf.generation, pf.seed = StubLib(), None, N_STUB, D_STUB, 0, SEED_STUB
    return pf


def run_key(seed, index):
    return int(load_library().cssm_pf_run_key(seed, (1 << 63) | index))


def test_native_pf_marshals_the_calls_and_the_default_keys():
    pf = stub_pf()
    for name in ("filter_forecasts", "filter_forecasts_more", "step_forecast", "forecasts_last_ms"):
        assert callable(getattr(NativePf, name)), name
    t, y, has = np.array([0.0, 1.0, 1.0, 2.5]), np.array([1.0, 0.0, 3.0, 2.0]), np.array([1, 0, 1, 1], dtype=np.uint8)
    r = pf.filter_forecasts(t, y, has, interval=0.9)
    c = pf.lib.calls[-1]
    assert c["name"] == "cssm_pf_filter_forecasts" and c["T"] == 4 and c["interval"] == 0.9 and c["keys"] is None and pf.generation == 1
    np.testing.assert_array_equal(c["t"], t); np.testing.assert_array_equal(c["y"], y); np.testing.assert_array_equal(c["has"], has)
    assert r["ll"] == 42.5 and list(r["ll_t"]) == [10.0, 11.0, 12.0, 13.0] and list(r["ess_t"]) == [20, 21, 22, 23]
    for j, name in enumerate(FORECAST_NAMES + ("obs_below", "obs_equal")):
        assert r[name].shape == ((4, D_STUB) if j < 3 else (4,)), name
        np.testing.assert_array_equal(r[name].ravel(), 1000 * (j + 1) + np.arange(r[name].size), err_msg=name)
    assert r["obs_below"].dtype == np.int32 and r["obs_equal"].dtype == np.int32
    # the keys a call without keys reports: cssm_pf_run_key(seed, 2^63 | index of the cloud before the record), a fresh call from index 0 ...
    assert [int(k) for k in r["keys"]] == [run_key(SEED_STUB, s) for s in range(4)]
    # ... a continued one from the handle's observation index
    r = pf.filter_forecasts_more(t, y)
    c = pf.lib.calls[-1]
    assert c["name"] == "cssm_pf_filter_forecasts_more" and c["has"] is None and c["interval"] == 0.975 and c["keys"] is None
    assert [int(k) for k in r["keys"]] == [run_key(SEED_STUB, INDEX_STUB + s) for s in range(4)]
    given = [3, 2**64 - 1, 7, 2**63]
    r = pf.filter_forecasts(t, y, has, keys=given)
    assert [int(k) for k in pf.lib.calls[-1]["keys"]] == given and [int(k) for k in r["keys"]] == given
    with pytest.raises(ValueError):
        pf.filter_forecasts(t, y, has, keys=[1, 2])
    ll, ess, fc = pf.step_forecast(3.0, None)
    c = pf.lib.calls[-1]
    assert (c["t"], c["y"], c["has"], c["use_key"], c["interval"]) == (3.0, 0.0, 0, 0, 0.975) and (ll, ess) == (-3.5, 9)
    assert fc["key"] == run_key(SEED_STUB, INDEX_STUB) == pf.forecast_key()
    assert fc["state_mean"].shape == (1, D_STUB) and fc["obs_mean"].shape == (1,) and fc["obs_below"][0] == 10000
    ll, ess, fc = pf.step_forecast(3.0, 2.0, key=2**64 - 3, interval=0.5)
    c = pf.lib.calls[-1]
    assert (c["y"], c["has"], c["key"], c["use_key"], c["interval"]) == (2.0, 1, 2**64 - 3, 1, 0.5) and fc["key"] == 2**64 - 3
    assert pf.forecasts_last_ms() == (3.0, 2.0)


def _stub_filter(cls, *extra):
    flt = cls(cases.c2_model(), Resampling.systematicResampling, *extra)
    flt._pf = stub_pf()
    flt._ensure = lambda n: flt._pf
    return flt


def _expect(t, r):
    from composablestatespacemodels_amd.filter import CredibleInterval
    return ForecastOut(t, 7000.0 + r, CredibleInterval(8000.0 + r, 9000.0 + r), 4000.0 + r, CredibleInterval(5000.0 + r, 6000.0 + r),
                       1000.0 + D_STUB * r + np.arange(D_STUB),
                       [CredibleInterval(2000.0 + D_STUB * r + k, 3000.0 + D_STUB * r + k) for k in range(D_STUB)])


def _same(a: ForecastOut, b: ForecastOut):
    import dataclasses
    da, db = dataclasses.asdict(a), dataclasses.asdict(b)
    for k in da:
        if isinstance(da[k], np.ndarray):
            np.testing.assert_array_equal(da[k], db[k])
        else:
            assert da[k] == db[k], k


def test_filter_and_filter_init_assemble_forecast_outs():
    assert callable(Filter.filterForecasts) and callable(Filter.stepForecast) and callable(FilterInit.filterForecasts)
    flt = _stub_filter(Filter)
    data = [Data(2.0, 1.0), Data(0.5, None), Data(3.0, 4.0)]
    ll, outs = flt.filterForecasts(data, N_STUB, interval=0.8)
    c = flt._pf.lib.calls[-1]
    assert c["name"] == "cssm_pf_filter_forecasts" and c["interval"] == 0.8 and list(c["has"]) == [1, 0, 1] and list(c["t"]) == [2.0, 0.5, 3.0]
    assert ll == 42.5 and len(outs) == 3
    for r, d in enumerate(data):
        _same(outs[r], _expect(d.t, r))
    st0 = flt._state(3.0, 4.0, ll, 5)
    st, out = flt.stepForecast(st0, Data(4.0, 2.0))
    assert (st.t, st.observation, st.ll, st.ess) == (4.0, 2.0, -3.5, 9) and st._generation == flt._pf.generation
    _same(out, _expect(4.0, 0))
    with pytest.raises(RuntimeError):
        flt.stepForecast(st0, Data(5.0, 1.0))                                             # not the current state any more
    fi = _stub_filter(FilterInit, [0.0, 0.1, 0.2])
    ll, outs = fi.filterForecasts(data, N_STUB)
    assert [c["name"] for c in fi._pf.lib.calls] == ["cssm_pf_init_from", "cssm_pf_filter_forecasts_more"]
    assert fi._pf.lib.calls[0]["t0"] == 0.5 and len(outs) == 3 and ll == 42.5


def test_the_cpp_surface_compiles_and_links(tmp_path):
    """include/cssm_pf.hpp: cssm::Filter::filterForecasts / filterForecastsMore / stepForecast with the stated signatures
    (tests/cpp/test_hpp_forecasts.cpp holds the static_asserts)."""
    lib = os.path.join(ROOT, "composablestatespacemodels_amd", "csrc")
    exe = str(tmp_path / "test_hpp_forecasts")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_hpp_forecasts.cpp"), "-L" + lib, "-lcssm_pf", "-Wl,-rpath," + lib, "-o", exe])
    assert os.path.exists(exe)


# ---- the premise: the selection with the observation row's ranks on the rows an observation draw produces --------------------------------
def count_rows(n: int):
    rng = np.random.default_rng(cases.SEED + 31 * n)
    rows = {f"poisson rate {lam}": rng.poisson(lam, n).astype(np.float64) for lam in (0.1, 2.0, 50.0)}
    rows["0/1 at p = 0.5"] = (rng.random(n) < 0.5).astype(np.float64)
    a = np.zeros(n); a[int(rng.integers(n))] = 1.0
    rows["0/1 at p = 1/N"] = a
    rows["one value only"] = np.full(n, 3.0)
    a = np.full(n, 2.0); a[n // 3] = 1e6
    rows["one outlier among equal values"] = a
    return rows


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("interval", INTERVALS)
def test_twin_selects_the_exact_order_statistics_of_count_like_rows(n, interval):
    _, cap, rounds, _ = twin_constants(n)
    for name, x in count_rows(n).items():
        got, st = twin_select(x, interval, state_row=False)           # the observation row: getOrderStatistic's ranks, as eta
        np.testing.assert_array_equal(_bits(got), _bits(exact_order_statistics(x, interval, False)), err_msg=name)
        assert st[0] <= rounds and st[2] <= cap and st[3] <= cap, (name, st)
