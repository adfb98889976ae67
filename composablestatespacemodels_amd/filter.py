"""Host-side mirror of the reference's particle-filter interface over libcssm_pf.

Reference (paths relative to src/main/scala/com/github/jonnylaw/model/):

* ``trait ParticleFilter[S]`` -- ParticleFilter.scala:96-167: ``initialiseState``, ``stepFilter``,
  ``llFilter``, ``filter``, ``filterStream``.
* ``Filter(mod, resample)`` :233-246, ``FilterInit(mod, resample, initState)`` :252-271,
  ``FilterLgcp(mod, resample, precision)`` :169-227.
* ``object ParticleFilter`` Reader entry points :321-361: ``filter``, ``filterInit``,
  ``filterLlState``, ``likelihood``; helpers ``effectiveSampleSize`` :431-434, ``mean`` :522-524.
* ``Resampling.systematicResampling`` -- Resampling.scala:63-72 (type ``Resample[A]``,
  package.scala:23).

Every computation happens in the HIP library; the particle cloud stays in HBM.  ``PfState`` is an
immutable value as in the reference (ParticleFilter.scala:32-37) except that ``particles`` is
fetched from the device on demand and is only available for the handle's CURRENT state.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass, field
from typing import Callable, Iterable, Iterator, List, Optional, Sequence, Tuple

import numpy as np

from . import _abi
from .model import Data, Model, Parameters, TimedObservation, UnparamModel, split_data

# the pointer an array is handed to the library as, by its dtype (an int32 array is a status or a count: `int*` / `int32_t*`, one type)
_PTR = {np.dtype(ty): C.POINTER(c) for ty, c in ((np.float64, C.c_double), (np.uint8, C.c_uint8), (np.int32, C.c_int), (np.uint32, C.c_uint32),
                                                 (np.uint64, C.c_uint64))}
_dp = _PTR[np.dtype(np.float64)]

FORECAST_NAMES = ("state_mean", "state_lower", "state_upper", "eta_mean", "eta_lower", "eta_upper", "obs_mean", "obs_lower", "obs_upper")


def _p(a, ty=None):
    """The array's address as the pointer its dtype names; None (an optional argument that is not given) stays None."""
    return None if a is None else a.ctypes.data_as(ty or _PTR[a.dtype])


def _u8(a):
    """An optional array of flags as the library takes it."""
    return None if a is None else np.ascontiguousarray(a, dtype=np.uint8)


def _filled(shape, fill):
    return np.zeros(shape) if fill == 0 else np.full(shape, fill)


def _interval_arrays(prefix, d, fill=0.0):
    """The six outputs of a summary in the C calls' order, preset to ``fill``: ``(state_mean, state_lower, state_upper)`` of shape
    ``[*prefix, d]`` and ``(eta_of_mean, eta_lower, eta_upper)`` of shape ``prefix``."""
    wide = (*prefix, d)
    return _filled(wide, fill), _filled(wide, fill), _filled(wide, fill), _filled(prefix, fill), _filled(prefix, fill), _filled(prefix, fill)


def _forecast_arrays(d, rows, fill=np.nan, pit=True):
    """The nine statistics of a forecast for ``rows`` rows, preset to ``fill`` -- with ``pit`` also the two PIT counts, preset to -1 -- by
    name, and their pointers in the C calls' order."""
    arr = {k: _filled((rows, d), fill) for k in FORECAST_NAMES[:3]}
    arr.update({k: _filled(rows, fill) for k in FORECAST_NAMES[3:]})
    if pit:
        arr.update({k: np.full(rows, -1, dtype=np.int32) for k in ("obs_below", "obs_equal")})
    return arr, [_p(v) for v in arr.values()]


class NativePf:
    """Thin RAII wrapper of a ``cssm_pf*`` handle (AutoCloseable on the Scala side)."""

    def __init__(self, model: Model, n: int, seed: int = 20260101, device: int = 0, lgcp_precision: int = 0):
        self.lib = _abi.load_library()
        self._desc = model.descriptor(lgcp_precision)
        self._h = C.c_void_p()
        _abi.check(self.lib.cssm_pf_create(self._desc.ptr(), int(n), int(seed) & (2**64 - 1), int(device), C.byref(self._h)))
        self.n = int(n)
        self.d = int(self.lib.cssm_pf_dim(self._h))
        self.generation = 0
        self.model = model
        self.seed = int(seed) & (2**64 - 1)
        # the same entry point bound once more with untyped pointers: run_more hands it raw array addresses
        self._ll_filter_more_raw = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, _dp,
                                               C.c_void_p, C.c_void_p)(("cssm_pf_ll_filter_more", self.lib))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self.lib.cssm_pf_destroy(self._h)
            self._h = C.c_void_p()

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def set_params(self, model: Model, lgcp_precision: int = 0):
        self._desc = model.descriptor(lgcp_precision)
        _abi.check(self.lib.cssm_pf_set_params(self._h, self._desc.ptr()))
        self.model = model

    def reseed(self, seed: int):
        _abi.check(self.lib.cssm_pf_reseed(self._h, int(seed) & (2**64 - 1)))
        self.seed = int(seed) & (2**64 - 1)

    def init(self, t0: float):
        _abi.check(self.lib.cssm_pf_init(self._h, float(t0)))
        self.generation += 1

    def init_from(self, t0: float, state: Sequence[float]):
        s = np.ascontiguousarray(state, dtype=np.float64)
        if s.size != self.d:
            raise ValueError(f"initial state has {s.size} components, the model has {self.d}")
        _abi.check(self.lib.cssm_pf_init_from(self._h, float(t0), _p(s)))
        self.generation += 1

    def step(self, t: float, y: Optional[float], has_obs: Optional[bool] = None) -> Tuple[float, int]:
        if has_obs is None:
            has_obs = y is not None
        ll, ess = C.c_double(), C.c_int32()
        rc = self.lib.cssm_pf_step(self._h, float(t), 0.0 if y is None else float(y), 1 if has_obs else 0,
                                   C.byref(ll), C.byref(ess))
        self.generation += 1
        _abi.check(rc)
        return ll.value, ess.value

    def propagate(self, t: float, y: Optional[float], has_obs: Optional[bool] = None):
        """cssm_pf_propagate: stepFilter up to the weights (the caller resamples: see _FilterBase with a host function)."""
        if has_obs is None:
            has_obs = y is not None
        rc = self.lib.cssm_pf_propagate(self._h, float(t), 0.0 if y is None else float(y), 1 if has_obs else 0)
        self.generation += 1
        _abi.check(rc)

    def adopt(self, state: np.ndarray, ll: float, ess: int):
        s = np.ascontiguousarray(state, dtype=np.float64)
        if s.shape != (self.d, self.n):
            raise ValueError(f"the resampled cloud must be [{self.d}, {self.n}], got {s.shape}")
        _abi.check(self.lib.cssm_pf_adopt(self._h, _p(s), float(ll), int(ess)))
        self.generation += 1

    def run(self, t, y, has=None, want_path: bool = False):
        t = np.ascontiguousarray(t, dtype=np.float64)
        y = np.ascontiguousarray(y, dtype=np.float64)
        T = len(t)
        has = _u8(has)
        ll = C.c_double()
        ll_t = np.zeros(T)
        ess_t = np.zeros(T, dtype=np.int32)
        path = None
        if want_path:
            path = np.zeros((T + 1, self.d))
            rc = self.lib.cssm_pf_filter(self._h, _p(t), _p(y), _p(has), T, C.byref(ll), _p(ll_t), _p(ess_t), _p(path))
        else:
            rc = self.lib.cssm_pf_ll_filter(self._h, _p(t), _p(y), _p(has), T, C.byref(ll), _p(ll_t), _p(ess_t))
        self.generation += 1
        _abi.check(rc)
        return ll.value, ll_t, ess_t, path

    def run_more(self, t, y, has=None):
        """T MORE observations of the running filter (cssm_pf_ll_filter_more): no new cloud, the clock and the observation count
        go on; returns (ll accumulated since initialisation, ll_t, ess_t) of this call's observations."""
        # (a short continued leg pays for every microsecond here: no copies of arrays that already are what the ABI takes, raw
        #  addresses instead of typed ctypes pointers)
        if not (type(t) is np.ndarray and t.dtype == np.float64 and t.flags.c_contiguous):
            t = np.ascontiguousarray(t, dtype=np.float64)
        if not (type(y) is np.ndarray and y.dtype == np.float64 and y.flags.c_contiguous):
            y = np.ascontiguousarray(y, dtype=np.float64)
        T = len(t)
        hp = None
        if has is not None:
            if not (type(has) is np.ndarray and has.dtype == np.uint8 and has.flags.c_contiguous):
                has = np.ascontiguousarray(has, dtype=np.uint8)
            hp = has.ctypes.data
        ll = C.c_double()
        ll_t = np.empty(T)
        ess_t = np.empty(T, dtype=np.int32)
        rc = self._ll_filter_more_raw(self._h, t.ctypes.data, y.ctypes.data, hp, T, C.byref(ll), ll_t.ctypes.data, ess_t.ctypes.data)
        self.generation += 1
        _abi.check(rc)
        return ll.value, ll_t, ess_t

    def last_loop_ms(self) -> float:
        """Device time of the last batch call's per-observation kernels; needs set_option(9, 1) (CSSM_OPT_LOOP_EVENTS) before that call."""
        ms = C.c_float()
        _abi.check(self.lib.cssm_pf_last_loop_ms(self._h, C.byref(ms)))
        return ms.value

    def last_device_us(self) -> float:
        """Device time of the last continued batch call, first instruction of its first kernel to its closing kernel's results, from the GPU's
        constant clock (cssm_pf_last_device_us: no event packets on the queue)."""
        us = C.c_double()
        _abi.check(self.lib.cssm_pf_last_device_us(self._h, C.byref(us)))
        return us.value

    def stream_idle(self) -> bool:
        """Whether the runtime sees nothing queued or running on the handle's stream (cssm_pf_stream_idle; raises on a HIP error)."""
        r = self.lib.cssm_pf_stream_idle(self._h)
        if r < 0:
            _abi.check(r)
        return r == 1

    KERNELS = ("k_propagate", "k_tile_sums", "k_offspring", "k_reduce_units", "k_boundary_pack", "k_offspring_expand_spec", "collective")

    def set_option(self, option: int, value: int):
        _abi.check(self.lib.cssm_pf_set_option(self._h, int(option), int(value)))

    def profile(self, enable: bool):
        _abi.check(self.lib.cssm_pf_profile(self._h, 1 if enable else 0))

    def profile_read(self):
        """{kernel: (total_ms, launches)} accumulated since profile(True)."""
        ms = np.zeros(len(self.KERNELS))
        cnt = np.zeros(len(self.KERNELS), dtype=np.uint64)
        _abi.check(self.lib.cssm_pf_profile_read(self._h, _p(ms), _p(cnt)))
        return {k: (float(ms[i]), int(cnt[i])) for i, k in enumerate(self.KERNELS)}

    def summary(self, interval: float = 0.975):
        """(state_mean[d], state_lower[d], state_upper[d], eta_of_mean, eta_lower, eta_upper) of the current cloud."""
        m, lo, hi = np.zeros(self.d), np.zeros(self.d), np.zeros(self.d)
        em, el, eu = C.c_double(), C.c_double(), C.c_double()
        _abi.check(self.lib.cssm_pf_summary(self._h, float(interval), _p(m), _p(lo), _p(hi), C.byref(em), C.byref(el), C.byref(eu)))
        return m, lo, hi, em.value, el.value, eu.value

    def _filter_intervals(self, fn, t, y, has, interval, nrows_extra):
        t = np.ascontiguousarray(t, dtype=np.float64)
        y = np.ascontiguousarray(y, dtype=np.float64)
        T = len(t)
        has = _u8(has)
        rows = _interval_arrays((T + nrows_extra,), self.d)
        ll = C.c_double()
        ll_t = np.zeros(T)
        ess_t = np.zeros(T, dtype=np.int32)
        rc = fn(self._h, _p(t), _p(y), _p(has), T, float(interval), C.byref(ll), _p(ll_t), _p(ess_t), *map(_p, rows))
        self.generation += 1
        _abi.check(rc)
        return (ll.value, ll_t, ess_t) + rows

    def filter_intervals(self, t, y, has=None, interval: float = 0.975):
        """cssm_pf_filter_intervals: ``run`` with the ``summary`` of the initial cloud (row 0) and of the cloud behind every record (row
        s + 1) from the same call: ``(ll, ll_t[T], ess_t[T], state_mean[T+1,d], state_lower, state_upper, eta_of_mean[T+1], eta_lower,
        eta_upper)``, every row with the bits of ``summary`` at that moment of the loop init; summary; (step; summary)*."""
        return self._filter_intervals(self.lib.cssm_pf_filter_intervals, t, y, has, interval, 1)

    def filter_intervals_more(self, t, y, has=None, interval: float = 0.975):
        """cssm_pf_filter_intervals_more: ``run_more`` with the ``summary`` behind every record: the same tuple with T rows (no initial row)."""
        return self._filter_intervals(self.lib.cssm_pf_filter_intervals_more, t, y, has, interval, 0)

    def step_intervals(self, t: float, y: Optional[float], has_obs: Optional[bool] = None, interval: float = 0.975):
        """cssm_pf_step_intervals: ``step`` and the ``summary`` of the cloud it leaves in one call: ``(ll, ess, state_mean[d], state_lower[d],
        state_upper[d], eta_of_mean, eta_lower, eta_upper)``."""
        if has_obs is None:
            has_obs = y is not None
        ll, ess = C.c_double(), C.c_int32()
        m, lo, hi = np.zeros(self.d), np.zeros(self.d), np.zeros(self.d)
        em, el, eu = C.c_double(), C.c_double(), C.c_double()
        rc = self.lib.cssm_pf_step_intervals(self._h, float(t), 0.0 if y is None else float(y), 1 if has_obs else 0, float(interval),
                                             C.byref(ll), C.byref(ess), _p(m), _p(lo), _p(hi), C.byref(em), C.byref(el), C.byref(eu))
        self.generation += 1
        _abi.check(rc)
        return ll.value, ess.value, m, lo, hi, em.value, el.value, eu.value

    def intervals_last_ms(self) -> Tuple[float, float]:
        """Device milliseconds of the last ``filter_intervals`` / ``filter_intervals_more`` / ``step_intervals``: (the whole call, its summary
        launches alone) (cssm_pf_intervals_last_ms)."""
        ms = np.zeros(2)
        _abi.check(self.lib.cssm_pf_intervals_last_ms(self._h, _p(ms)))
        return float(ms[0]), float(ms[1])

    def observation_index(self) -> int:
        """Observations the current cloud has seen (cssm_pf_observation_index)."""
        return int(self.lib.cssm_pf_observation_index(self._h))

    def forecast_key(self) -> int:
        """The default Philox key of a forecast of the current cloud: cssm_pf_run_key(seed, 2^63 | observation index) -- two forecasts
        of one state draw the same, forecasts of different states different streams, none the filter's own."""
        return int(self.lib.cssm_pf_run_key(self.seed, (1 << 63) | self.observation_index()))

    def forecast(self, t, key: Optional[int] = None, interval: float = 0.975, want_samples: bool = False):
        """cssm_pf_forecast over the times t[0..H): dict of per-horizon arrays state_mean / state_lower / state_upper [H, d],
        eta_mean / eta_lower / eta_upper / obs_mean / obs_lower / obs_upper [H], and with want_samples samples [H, d + 3, N]
        (rows: the d states, gamma, eta, obs).  The filter itself is not touched (its generation does not change)."""
        t = np.ascontiguousarray(np.atleast_1d(np.asarray(t, dtype=np.float64)))
        H = len(t)
        key = self.forecast_key() if key is None else int(key) & (2**64 - 1)
        out, ptrs = _forecast_arrays(self.d, H, 0.0, pit=False)
        samples = np.zeros((H, self.d + 3, self.n)) if want_samples else None
        _abi.check(self.lib.cssm_pf_forecast(self._h, _p(t), H, key, float(interval), *ptrs, _p(samples)))
        out["samples"] = samples
        out["key"] = key
        return out

    def default_forecast_keys(self, first_index: int, count: int) -> np.ndarray:
        """The keys ``forecast_key`` returns for the clouds of observation indices first_index .. first_index + count - 1."""
        return np.array([int(self.lib.cssm_pf_run_key(self.seed, (1 << 63) | (int(first_index) + s))) for s in range(count)], dtype=np.uint64)

    def _filter_forecasts(self, fn, t, y, has, keys, interval, first_index):
        t = np.ascontiguousarray(t, dtype=np.float64)
        y = np.ascontiguousarray(y, dtype=np.float64)
        T = len(t)
        has = _u8(has)
        if keys is None:
            used, ky = self.default_forecast_keys(first_index, T), None
        else:
            ky = used = np.ascontiguousarray([int(x) & (2**64 - 1) for x in np.asarray(keys, dtype=object).ravel()], dtype=np.uint64)
            if len(ky) != T:
                raise ValueError(f"one key per record ({T}), not {len(ky)}")
        out, ptrs = _forecast_arrays(self.d, T)
        ll = C.c_double()
        ll_t = np.zeros(T)
        ess_t = np.zeros(T, dtype=np.int32)
        rc = fn(self._h, _p(t), _p(y), _p(has), T, _p(ky), float(interval), C.byref(ll), _p(ll_t), _p(ess_t), *ptrs)
        self.generation += 1
        _abi.check(rc)
        out.update(ll=ll.value, ll_t=ll_t, ess_t=ess_t, keys=used)
        return out

    def filter_forecasts(self, t, y, has=None, keys=None, interval: float = 0.975):
        """cssm_pf_filter_forecasts: ``run`` and, from the same call, before every record is stepped, ``forecast`` of the record's time
        from the cloud before it (``ParticleFilter.getMeanForecast`` mapped over the filter stream).  ``forecast``'s dict with [T] rows
        (state_* [T, d]) plus ``ll``, ``ll_t``, ``ess_t``, the PIT counts ``obs_below`` / ``obs_equal`` (draws strictly below / equal to
        the datum; -1 without one) and ``keys`` (the Philox key of every row; ``keys=None``: the rule of ``forecast_key`` per record).
        A record whose time ``forecast`` would refuse reads NaN and -1."""
        return self._filter_forecasts(self.lib.cssm_pf_filter_forecasts, t, y, has, keys, interval, 0)

    def filter_forecasts_more(self, t, y, has=None, keys=None, interval: float = 0.975):
        """cssm_pf_filter_forecasts_more: ``run_more`` with the forecast before every record: the same dict."""
        return self._filter_forecasts(self.lib.cssm_pf_filter_forecasts_more, t, y, has, keys, interval, self.observation_index())

    def step_forecast(self, t: float, y: Optional[float], has_obs: Optional[bool] = None, key: Optional[int] = None, interval: float = 0.975):
        """cssm_pf_step_forecast: ``forecast([t], key)`` of the current cloud, then ``step``, in one call: ``(ll, ess, fc)``; ``fc`` is
        ``forecast``'s dict with one row ([1, d] / [1]), the PIT counts and ``key`` (None: ``forecast_key()``)."""
        if has_obs is None:
            has_obs = y is not None
        used = self.forecast_key() if key is None else int(key) & (2**64 - 1)
        out, ptrs = _forecast_arrays(self.d, 1)
        ll, ess = C.c_double(), C.c_int32()
        rc = self.lib.cssm_pf_step_forecast(self._h, float(t), 0.0 if y is None else float(y), 1 if has_obs else 0, used if key is not None else 0,
                                            0 if key is None else 1, float(interval), C.byref(ll), C.byref(ess), *ptrs)
        self.generation += 1
        _abi.check(rc)
        out["key"] = used
        return ll.value, ess.value, out

    def forecasts_last_ms(self) -> Tuple[float, float]:
        """Device milliseconds of the last ``filter_forecasts`` / ``filter_forecasts_more`` / ``step_forecast``: (the whole call, its forecast
        rows' launches alone) (cssm_pf_forecasts_last_ms)."""
        ms = np.zeros(2)
        _abi.check(self.lib.cssm_pf_forecasts_last_ms(self._h, _p(ms)))
        return float(ms[0]), float(ms[1])

    def forecast_posterior(self, theta, x, t0: float, times, key: Optional[int] = None, interval: float = 0.975, pick=None,
                           want_samples: bool = False):
        """cssm_pf_forecast_posterior: forecasts from a joint posterior sample of M pairs -- theta[M, n_theta] in flatten order and
        x[M, d], their states at t0 -- with this handle's N particles, particle i on pair pick[i] (drawn under `key` when pick is
        None).  The same dict as ``forecast``, plus pick[N] (uint32).  The handle's model gives the structure; its cloud, time and
        parameters are not used or touched."""
        theta = np.ascontiguousarray(np.atleast_2d(np.asarray(theta, dtype=np.float64)))
        x = np.ascontiguousarray(np.asarray(x, dtype=np.float64).reshape(theta.shape[0], -1))
        M, nt = theta.shape
        if x.shape != (M, self.d):
            raise ValueError(f"x must be M x d = {M} x {self.d} (got {x.shape})")
        t = np.ascontiguousarray(np.atleast_1d(np.asarray(times, dtype=np.float64)))
        H = len(t)
        key = self.forecast_key() if key is None else int(key) & (2**64 - 1)
        pk = None
        if pick is not None:
            p = np.asarray(pick)
            if p.shape != (self.n,) or (p < 0).any():
                raise ValueError(f"pick must hold N = {self.n} non-negative indices")
            pk = np.ascontiguousarray(p, dtype=np.uint32)
        out, ptrs = _forecast_arrays(self.d, H, 0.0, pit=False)
        samples = np.zeros((H, self.d + 3, self.n)) if want_samples else None
        pick_out = np.zeros(self.n, dtype=np.uint32)
        _abi.check(self.lib.cssm_pf_forecast_posterior(self._h, self._desc.ptr(), _p(theta), nt, _p(x), M, float(t0), _p(t), H, _p(pk), key,
                                                       float(interval), *ptrs, _p(samples), _p(pick_out)))
        out["samples"] = samples
        out["key"] = key
        out["pick"] = pick_out
        return out

    def forecast_last_ms(self) -> Tuple[float, float]:
        """(k_forecast, selection) device milliseconds of the last forecast (cssm_pf_forecast_last_ms)."""
        ms = np.zeros(2)
        _abi.check(self.lib.cssm_pf_forecast_last_ms(self._h, _p(ms)))
        return float(ms[0]), float(ms[1])

    def interpolate(self, t, y, has=None, interval: float = 0.975, reference_pairing: bool = False):
        """cssm_pf_interpolate: (ll, mean[T+1,d], lower, upper, eta_of_mean[T+1], eta_lower, eta_upper)."""
        t = np.ascontiguousarray(t, dtype=np.float64)
        y = np.ascontiguousarray(y, dtype=np.float64)
        T = len(t)
        has = _u8(has)
        rows = _interval_arrays((T + 1,), self.d)
        ll = C.c_double()
        rc = self.lib.cssm_pf_interpolate(self._h, _p(t), _p(y), _p(has), T, float(interval), 1 if reference_pairing else 0,
                                          C.byref(ll), *map(_p, rows))
        self.generation += 1
        _abi.check(rc)
        return (ll.value,) + rows

    def smooth(self, t, y, has=None, n_traj: Optional[int] = None, interval: float = 0.975, want_trajectories: bool = False):
        """cssm_pf_smooth (an EXTENSION: the reference has no smoother beyond ``FilterInterpolate``): ``interpolate``'s forward pass, then
        ``n_traj`` trajectories (None: min(N, 4096)) drawn backwards through the kept clouds and summarised per time index.  Returns what
        ``interpolate`` returns, ``(ll, mean[T+1,d], lower, upper, eta_of_mean[T+1], eta_lower, eta_upper)``, and with
        ``want_trajectories`` one more entry: the uint32 array ``[T + 1, n_traj]`` of the particle of each kept cloud every trajectory
        passes through.  The handle must be re-initialised before further streaming calls."""
        M = min(self.n, _abi.FLEET_MAX_N) if n_traj is None else int(n_traj)
        if not 1 <= M <= _abi.FLEET_MAX_N:
            raise ValueError(f"n_traj must be in [1, {_abi.FLEET_MAX_N}], not {M}")
        if not 0.0 < float(interval) <= 1.0:
            raise ValueError(f"interval must be in (0, 1], not {interval}")
        t = np.ascontiguousarray(t, dtype=np.float64)
        y = np.ascontiguousarray(y, dtype=np.float64)
        T = len(t)
        has = _u8(has)
        rows = _interval_arrays((T + 1,), self.d)
        traj = np.zeros((T + 1, M), dtype=np.uint32) if want_trajectories else None
        ll = C.c_double()
        rc = self.lib.cssm_pf_smooth(self._h, _p(t), _p(y), _p(has), T, M, float(interval), 0, C.byref(ll), *map(_p, rows), _p(traj))
        self.generation += 1
        _abi.check(rc)
        out = (ll.value,) + rows
        return out + (traj,) if want_trajectories else out

    def smooth_last_ms(self) -> Tuple[float, float, float]:
        """Device time (HIP events) of the last ``smooth``'s forward pass, backward simulation and row summaries, ms."""
        ms = np.zeros(3)
        _abi.check(self.lib.cssm_pf_smooth_last_ms(self._h, _p(ms)))
        return float(ms[0]), float(ms[1]), float(ms[2])

    def if2(self, t, y, has, rw_sd, cooling: float, iters: int, seed: int, theta0=None, swarm0=None, first_iter: int = 0,
            want_swarm: bool = False, want_last: bool = False):
        """cssm_pf_if2 (an EXTENSION: the reference has no likelihood maximiser): one search of iterated filtering with the handle's N
        particles, from the row ``theta0[n_theta]`` (or the swarm ``swarm0[n_theta, N]`` of an earlier call, continued at ``first_iter``)
        under ``seed``; ``rw_sd[n_theta]`` the random-walk standard deviations, ``cooling`` the factor they shrink by over 50
        iterations.  Returns a dict with the keys of one series of ``NativePfFleet.if2``: ``theta_mean[iters, n_theta]``, ``ll[iters]``,
        ``rc`` (-5: some record left no particle a usable weight; the rows read NaN from that iteration on -- a status, not an
        exception); with ``want_swarm`` also ``swarm[n_theta, N]``; with ``want_last`` the last iteration's ``ll_t[T]``, ``ess_t[T]``,
        ``x[d, N]`` and ``anc[N]``.  The handle is only lent: its cloud, clock, key and options are afterwards what they were."""
        if theta0 is None and swarm0 is None:
            raise ValueError("theta0 (a starting row) or swarm0 (a whole swarm) is needed")
        sd = np.ascontiguousarray(rw_sd, dtype=np.float64)
        if sd.ndim != 1:
            raise ValueError("rw_sd must be a vector of n_theta standard deviations")
        nt = int(sd.shape[0])
        th0 = None if theta0 is None else np.ascontiguousarray(theta0, dtype=np.float64).reshape(nt)
        sw0 = None if swarm0 is None else np.ascontiguousarray(swarm0, dtype=np.float64).reshape(nt, self.n)
        t = np.ascontiguousarray(t, dtype=np.float64)
        y = np.ascontiguousarray(y, dtype=np.float64)
        T = len(t)
        if len(y) != T:
            raise ValueError("t and y must have one entry per record")
        has = _u8(has)
        iters = int(iters)
        out = {"theta_mean": np.full((max(iters, 0), nt), np.nan), "ll": np.full(max(iters, 0), np.nan)}
        swarm = np.zeros((nt, self.n)) if want_swarm else None
        ll_t, ess_t = (np.zeros(max(T, 1)), np.zeros(max(T, 1), dtype=np.int32)) if want_last else (None, None)
        x, anc = (np.zeros((self.d, self.n)), np.zeros(self.n, dtype=np.uint32)) if want_last else (None, None)
        rc = self.lib.cssm_pf_if2(self._h, _p(th0), _p(sw0), nt, _p(sd), float(cooling), int(first_iter), iters, int(seed) & (2**64 - 1),
                                  _p(t), _p(y), _p(has), T, _p(out["theta_mean"]), _p(out["ll"]), _p(swarm), _p(ll_t), _p(ess_t), _p(x), _p(anc))
        if rc != _abi.CSSM_ENONFINITE:
            _abi.check(rc)
        out["rc"] = int(rc)
        if want_swarm:
            out["swarm"] = swarm
        if want_last:
            out.update(ll_t=ll_t[:T], ess_t=ess_t[:T], x=x, anc=anc)
        return out

    def if2_last_ms(self) -> float:
        """Device time (HIP events) of the launches of the last ``if2``, ms."""
        ms = np.zeros(1)
        _abi.check(self.lib.cssm_pf_if2_last_ms(self._h, _p(ms)))
        return float(ms[0])

    def window(self, slices: int):
        """cssm_pf_window: remember the ``slices`` most recent clouds and ancestor arrays on the device (slices x stride x (8 d + 4) bytes)
        for ``step_interpolate``; 0 frees them.  Every call restarts the window."""
        if not 0 <= int(slices) < _abi.CSSM_PF_NO_ROWS:
            raise ValueError("slices must be in 0 .. 2^32 - 2")
        _abi.check(self.lib.cssm_pf_window(self._h, int(slices)))

    def window_depth(self) -> int:
        """The records remembered behind the window's base slice (cssm_pf_window_depth): 0 .. slices - 1."""
        return int(self.lib.cssm_pf_window_depth(self._h))

    def step_interpolate(self, t: float, y: Optional[float], has_obs: Optional[bool] = None, lag: Optional[int] = None, interval: float = 0.975):
        """cssm_pf_step_interpolate: ``step``, which also remembers the cloud it proposed in the handle's window, and the fixed-lag
        interpolation behind it: ``(ll, ess, nrows, (state_mean[lag + 1, d], state_lower, state_upper, eta_of_mean[lag + 1], eta_lower,
        eta_upper))``.  Row j summarises time index (newest - j) through the lineages that survive to the cloud just written; ``nrows`` =
        min(lag, window_depth()) + 1 rows are filled, the others read NaN.  ``lag=None``: step and remember only -- ``nrows`` = 0 and
        six arrays of one NaN row that the call does not touch."""
        if has_obs is None:
            has_obs = y is not None
        if lag is not None and not 0 <= int(lag) < _abi.CSSM_PF_NO_ROWS:
            raise ValueError("lag must be in 0 .. 2^32 - 2 (None asks for no rows)")
        ll, ess, nrows = C.c_double(), C.c_int32(), C.c_uint32()
        rows = _interval_arrays(((0 if lag is None else int(lag)) + 1,), self.d, np.nan)
        rc = self.lib.cssm_pf_step_interpolate(self._h, float(t), 0.0 if y is None else float(y), 1 if has_obs else 0,
                                               _abi.CSSM_PF_NO_ROWS if lag is None else int(lag), float(interval), C.byref(ll), C.byref(ess),
                                               C.byref(nrows), *map(_p, rows))
        self.generation += 1
        _abi.check(rc)
        return ll.value, ess.value, int(nrows.value), rows

    def step_interpolate_last_ms(self) -> Tuple[float, float]:
        """Device milliseconds of the last ``step_interpolate``: (the whole call, its row launches alone -- 0 without rows)
        (cssm_pf_step_interpolate_last_ms)."""
        ms = np.zeros(2)
        _abi.check(self.lib.cssm_pf_step_interpolate_last_ms(self._h, _p(ms)))
        return float(ms[0]), float(ms[1])

    def particles(self) -> np.ndarray:
        out = np.zeros((self.d, self.n))
        _abi.check(self.lib.cssm_pf_get_particles(self._h, _p(out)))
        return out

    def proposed(self) -> np.ndarray:
        out = np.zeros((self.d, self.n))
        _abi.check(self.lib.cssm_pf_get_proposed(self._h, _p(out)))
        return out

    def weights(self):
        """(w1, c): the weights exp(min(w - c, 2^-20)) of the last weighted step and the level c they are relative to -- what the
        fused kernel keeps in place of the log-weights; None where the handle keeps log-weights (see ``logw``)."""
        out = np.zeros(self.n)
        level = C.c_double()
        rc = self.lib.cssm_pf_get_weights(self._h, _p(out), C.byref(level))
        if rc == -7:       # CSSM_ESTATE: log-weights are kept
            return None
        _abi.check(rc)
        return out, level.value

    def logw(self) -> np.ndarray:
        out = np.zeros(self.n)
        _abi.check(self.lib.cssm_pf_get_logw(self._h, _p(out)))
        return out

    def ancestors(self) -> np.ndarray:
        out = np.zeros(self.n, dtype=np.uint32)
        _abi.check(self.lib.cssm_pf_get_ancestors(self._h, _p(out)))
        return out


# --------------------------------------------------------------------------- Resample[A]
class NativePfBatch:
    """``cssm_pfb*``: B filters of one model structure advanced in lockstep, one launch per stage for all of them (the chains of a PMMH
    run, a pilot grid of parameters -- model/Streaming.scala:38-39).  ``filter(models, seeds, t, y, has)`` = B x ``NativePf.run(...,
    want_path=True)`` on handles reseeded with ``seeds[k]``, bit for bit."""

    def __init__(self, model: Model, n: int, chains: int, device: int = 0):
        self.lib = _abi.load_library()
        self._h = C.c_void_p()
        self._desc = model.descriptor()
        _abi.check(self.lib.cssm_pfb_create(self._desc.ptr(), int(n), int(chains), int(device), C.byref(self._h)))
        self.B, self.n = int(chains), int(n)
        self.d = int(self.lib.cssm_pf_dim(self.lib.cssm_pfb_chain(self._h, 0)))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self.lib.cssm_pfb_destroy(self._h)
            self._h = C.c_void_p()

    __del__ = close

    def filter(self, models: Sequence[Model], seeds: Sequence[int], t, y, has=None, want_path: bool = True):
        """(ll[B], path[B, T + 1, d] or None, rc[B]): rc[k] != 0 is chain k's own status (-5: its weights were unusable)."""
        if len(models) != self.B or len(seeds) != self.B:
            raise ValueError("one model and one seed per chain")
        t = np.ascontiguousarray(t, dtype=np.float64); y = np.ascontiguousarray(y, dtype=np.float64)
        T = len(t)
        has = _u8(has)
        descs = [m.descriptor() for m in models]
        arr = (_abi._descp * self.B)(*[C.pointer(d.desc) for d in descs])
        sd = np.ascontiguousarray([int(x) & (2**64 - 1) for x in seeds], dtype=np.uint64)
        ll = np.zeros(self.B); rc = np.zeros(self.B, dtype=np.int32)
        path = np.zeros((self.B, T + 1, self.d)) if want_path else None
        _abi.check(self.lib.cssm_pfb_filter(self._h, arr, _p(sd), _p(t), _p(y), _p(has), T, _p(ll), _p(path), _p(rc)))
        return ll, path, rc

    def chain(self, k: int) -> "NativePf":
        """Chain k as a NativePf view (inspection only; the batch owns the handle)."""
        v = _PfView.__new__(_PfView)
        v.lib = self.lib; v._h = C.c_void_p(self.lib.cssm_pfb_chain(self._h, int(k))); v.n = self.n; v.d = self.d; v.generation = 0
        v.model = None; v.seed = 0; v._desc = self._desc
        return v


class NativePfFleet:
    """``cssm_fleet*``: S series of one model structure, N <= ``_abi.FLEET_MAX_N`` particles each, parameters / key / data / clock of
    its own per series; ONE launch advances all of them, one workgroup per series (include/cssm_pf.h, "fleet of independent
    series").  Per series every result has the bits of a ``NativePf`` of its own."""

    _CREATE = "cssm_fleet_create"          # the call that makes the handle (NativeLgcpFleet: cssm_fleet_create_lgcp)

    def __init__(self, model: Model, n: int, series: int, device: int = 0):
        self.lib = _abi.load_library()
        self._h = C.c_void_p()
        self._desc = self._descriptor(model)
        _abi.check(getattr(self.lib, self._CREATE)(self._desc.ptr(), int(n), int(series), int(device), C.byref(self._h)))
        self.S, self.n = int(series), int(n)
        words = (C.c_uint32 * (_abi.MAX_DIM // 4))()
        d = C.c_int32()
        _abi.check(self.lib.cssm_model_structure(self._desc.ptr(), words, C.byref(d)))
        self.d = int(d.value)
        nt = C.c_size_t()
        _abi.check(self.lib.cssm_desc_flatten(self._desc.ptr(), None, 0, C.byref(nt)))
        self.n_theta = int(nt.value)       # the length of a parameter row in flatten order
        self.generation = 0
        self.seeds = [0] * self.S          # the keys given to reseed (cssm_fleet_reseed's default: 0)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self.lib.cssm_fleet_destroy(self._h)
            self._h = C.c_void_p()

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _descriptor(self, model: Model):
        """The descriptor a model is handed to the library as (NativeLgcpFleet: with the fleet's precision)."""
        return model.descriptor()

    def set_params(self, models: Sequence[Model]):
        if len(models) != self.S:
            raise ValueError("one model per series")
        cache = {}
        descs = [cache.setdefault(id(m), self._descriptor(m)) for m in models]   # (pointers may repeat)
        arr = (_abi._descp * self.S)(*[C.pointer(d.desc) for d in descs])
        _abi.check(self.lib.cssm_fleet_set_params(self._h, arr))

    def reseed(self, seeds: Sequence[int]):
        if len(seeds) != self.S:
            raise ValueError("one seed per series")
        sd = np.ascontiguousarray([int(x) & (2**64 - 1) for x in seeds], dtype=np.uint64)
        _abi.check(self.lib.cssm_fleet_reseed(self._h, _p(sd)))
        self.seeds = [int(x) for x in sd]

    def set_option(self, option: int, value: int):
        _abi.check(self.lib.cssm_fleet_set_option(self._h, int(option), int(value)))

    @staticmethod
    def pack(datas, allow_empty: bool = False):
        """The ragged arrays of ``cssm_fleet_ll_filter`` from a sequence of ``(t, y, has)`` triples (``has`` may be None = all
        observed): ``(off uint64[S + 1], t, y, has uint8)``, C-contiguous.  An empty series is refused here, before any device call
        (the reference's ``minBy`` throws on an empty Vector) -- unless ``allow_empty`` (``interpolate``: the series' own status says
        so, the others run)."""
        off = np.zeros(len(datas) + 1, dtype=np.uint64)
        ts, ys, hs = [], [], []
        for k, tr in enumerate(datas):
            t, y = np.asarray(tr[0], dtype=np.float64).ravel(), np.asarray(tr[1], dtype=np.float64).ravel()
            h = tr[2] if len(tr) > 2 else None
            h = np.ones(len(t), dtype=np.uint8) if h is None else np.asarray(h, dtype=np.uint8).ravel()
            if len(t) == 0 and not allow_empty:
                raise ValueError(f"series {k} has no records (the reference's minBy throws on an empty Vector)")
            if len(y) != len(t) or len(h) != len(t):
                raise ValueError(f"series {k}: t, y and has differ in length")
            off[k + 1] = off[k] + np.uint64(len(t))
            ts.append(t); ys.append(y); hs.append(h)

        def cat(v, ty):
            return np.ascontiguousarray(np.concatenate(v) if v else np.zeros(0), dtype=ty)
        return off, cat(ts, np.float64), cat(ys, np.float64), cat(hs, np.uint8)

    def ll_filter(self, datas):
        """llFilter of every series: ``(ll[S], [ll_t of series k], [ess_t of series k], rc[S])``; rc[k] != 0 is series k's own status
        (-5: its weights were unusable; its later ll_t read NaN)."""
        if len(datas) != self.S:
            raise ValueError("one (t, y, has) triple per series")
        return self.ll_filter_packed(*self.pack(datas))

    def ll_filter_packed(self, off, t, y, has):
        """``ll_filter`` on arrays ``pack`` made (a caller that filters the same fleet repeatedly packs once)."""
        R, t, y, has = self._record_inputs(off, t, y, has)
        ll, rc, ll_t, ess_t = self._record_outputs(R)
        self.generation += 1
        _abi.check(self.lib.cssm_fleet_ll_filter(self._h, _p(off), _p(t), _p(y), _p(has), _p(ll), _p(ll_t), _p(ess_t), _p(rc)))
        return ll, self._split(off, ll_t), self._split(off, ess_t), rc

    def _check_packed(self, off, t, y, has):
        """What every packed call refuses before any device call: a ragged layout that is not S series of t / y / has."""
        off = np.asarray(off)
        if off.dtype != np.uint64 or off.ndim != 1 or len(off) != self.S + 1:
            raise ValueError(f"off must hold S + 1 = {self.S + 1} uint64 offsets")
        if int(off[0]) != 0 or (off[1:] < off[:-1]).any():
            raise ValueError("off[0] must be 0 and off must be non-decreasing")
        R = int(off[-1])
        for name, a, ty in (("t", t, np.float64), ("y", y, np.float64), ("has", has, np.uint8)):
            if a is None or a.dtype != ty or len(a) != R or not a.flags.c_contiguous:
                raise ValueError(f"{name} must be a C-contiguous {np.dtype(ty).name} array of off[-1] = {R} entries")
        return R

    def _record_inputs(self, off, t, y, has):
        """What every packed record call starts with: ``_check_packed``, then ``(R, t, y, has)`` as the C call takes them -- it refuses null
        data, so a fleet without a single record hands over one-entry placeholders, which are never read."""
        R = self._check_packed(off, t, y, has)
        return (R, t, y, has) if R else (0, np.zeros(1), np.zeros(1), np.zeros(1, dtype=np.uint8))

    def _record_outputs(self, R):
        """``(ll[S], rc[S], ll_t[R], ess_t[R])`` of a record call."""
        return np.zeros(self.S), np.zeros(self.S, dtype=np.int32), np.zeros(R), np.zeros(R, dtype=np.int32)

    @staticmethod
    def _split(off, a, extra=0):
        """Series k's rows of ``a``, per series: ``off[k] + extra k .. off[k + 1] + extra (k + 1)`` -- ``extra`` = 0 for an array laid out
        like the records, 1 for one laid out like the paths (T_k + 1 rows per series, row 0 the initial cloud)."""
        first = [v + extra * k for k, v in enumerate(np.asarray(off).tolist())]
        return [a[i:j] for i, j in zip(first, first[1:])]

    @classmethod
    def _split_named(cls, off, arr):
        """``_split`` of every array of a dict: per series a dict of its rows under the same names."""
        per = {name: cls._split(off, v) for name, v in arr.items()}
        return [{name: rows[k] for name, rows in per.items()} for k in range(len(off) - 1)]

    def ll_filter_more(self, datas):
        """cssm_fleet_ll_filter_more: T_k MORE records of every running series in one launch -- ``NativePf.run_more`` per series, what a
        loop of ``step`` does with a launch per record.  ``datas[k]`` may be empty (the series is left alone).  ``(ll[S], [ll_t of series
        k], [ess_t of series k], rc[S])``: ll[k] accumulated since the series was initialised (NaN for a series the call did not advance);
        rc[k] -7: records for a series without a cloud, -5: its weights were unusable."""
        if len(datas) != self.S:
            raise ValueError("one (t, y, has) triple per series")
        return self.ll_filter_more_packed(*self.pack(datas, allow_empty=True))

    def ll_filter_more_packed(self, off, t, y, has):
        """``ll_filter_more`` on arrays ``pack`` made."""
        R, t, y, has = self._record_inputs(off, t, y, has)
        ll, rc, ll_t, ess_t = self._record_outputs(R)
        ll[:] = np.nan
        self.generation += 1
        _abi.check(self.lib.cssm_fleet_ll_filter_more(self._h, _p(off), _p(t), _p(y), _p(has), _p(ll), _p(ll_t), _p(ess_t), _p(rc)))
        return ll, self._split(off, ll_t), self._split(off, ess_t), rc

    def filter_intervals_more(self, datas, interval: float = 0.975):
        """cssm_fleet_filter_intervals_more: ``ll_filter_more`` and, from the same launch, ``summary`` of the cloud after every record:
        ``(ll[S], [ll_t of series k], [ess_t of series k], per-series list of (mean[T_k, d], lower, upper, eta_of_mean[T_k], eta_lower,
        eta_upper), rc[S])`` -- a row per record, none for an initial cloud; rows behind a failing record and of a series without a cloud
        read NaN."""
        if len(datas) != self.S:
            raise ValueError("one (t, y, has) triple per series")
        return self.filter_intervals_more_packed(*self.pack(datas, allow_empty=True), interval=interval)

    def filter_intervals_more_packed(self, off, t, y, has, interval: float = 0.975):
        """``filter_intervals_more`` on arrays ``pack`` made."""
        R, t, y, has = self._record_inputs(off, t, y, has)
        ll, rc, ll_t, ess_t = self._record_outputs(R)
        ll[:] = np.nan
        rows = _interval_arrays((R,), self.d)
        self.generation += 1
        _abi.check(self.lib.cssm_fleet_filter_intervals_more(self._h, _p(off), _p(t), _p(y), _p(has), float(interval), _p(ll), _p(ll_t), _p(ess_t),
                                                             *map(_p, rows), _p(rc)))
        per = [self._split(off, a) for a in rows]
        return ll, self._split(off, ll_t), self._split(off, ess_t), [tuple(r[k] for r in per) for k in range(self.S)], rc

    def filter(self, datas, want_path: bool = True):
        """``filter`` of every series (cssm_fleet_filter): ``(ll[S], [ll_t of series k], [ess_t of series k], paths, last[S, d], rc[S])``.
        ``paths``: a list of ``[T_k + 1, d]`` arrays -- row 0 the sampled particle of the initial cloud, row s + 1 the one after
        observation s -- or None without ``want_path`` (the device then keeps and returns the last rows only).  A series whose rc is
        not zero reads NaN from the failing observation on and in its ``last`` row."""
        if len(datas) != self.S:
            raise ValueError("one (t, y, has) triple per series")
        return self.filter_packed(*self.pack(datas), want_path=want_path)

    def filter_packed(self, off, t, y, has, want_path: bool = True):
        """``filter`` on arrays ``pack`` made (a caller that filters the same fleet repeatedly packs once)."""
        R, t, y, has = self._record_inputs(off, t, y, has)
        ll, rc, ll_t, ess_t = self._record_outputs(R)
        last = np.zeros((self.S, self.d))
        path = np.zeros((R + self.S, self.d)) if want_path else None
        self.generation += 1
        _abi.check(self.lib.cssm_fleet_filter(self._h, _p(off), _p(t), _p(y), _p(has), _p(ll), _p(ll_t), _p(ess_t), _p(path), _p(last), _p(rc)))
        return ll, self._split(off, ll_t), self._split(off, ess_t), self._split(off, path, 1) if want_path else None, last, rc

    def filter_intervals(self, datas, interval: float = 0.975):
        """cssm_fleet_filter_intervals: ``ll_filter`` and, from the same launch, ``summary`` of the initial cloud and of the cloud after
        every record.  ``(ll[S], [ll_t of series k], [ess_t of series k], per-series list of (mean[T_k + 1, d], lower, upper,
        eta_of_mean[T_k + 1], eta_lower, eta_upper), rc[S])``; rc[k] != 0 is series k's own status (-6: no records, its single row reads
        NaN; -5: its weights were unusable at observation s, its rows read NaN from s + 1 on).  The fleet continues with ``step``."""
        if len(datas) != self.S:
            raise ValueError("one (t, y, has) triple per series")
        return self.filter_intervals_packed(*self.pack(datas, allow_empty=True), interval=interval)

    def filter_intervals_packed(self, off, t, y, has, interval: float = 0.975):
        """``filter_intervals`` on arrays ``pack`` made (a caller that filters the same fleet repeatedly packs once)."""
        R, t, y, has = self._record_inputs(off, t, y, has)
        ll, rc, ll_t, ess_t = self._record_outputs(R)
        rows = _interval_arrays((R + self.S,), self.d)
        self.generation += 1
        _abi.check(self.lib.cssm_fleet_filter_intervals(self._h, _p(off), _p(t), _p(y), _p(has), float(interval), _p(ll), _p(ll_t), _p(ess_t),
                                                        *map(_p, rows), _p(rc)))
        return ll, self._split(off, ll_t), self._split(off, ess_t), self.interpolate_rows(off, rows), rc

    FORECAST_NAMES = FORECAST_NAMES

    def _forecast_arrays(self, rows: int, fill=np.nan, pit: bool = True):
        """The nine statistics of ``forecast`` for ``rows`` rows, preset to ``fill`` -- with ``pit`` also the two PIT counts, preset to -1 --
        and their pointers in the C calls' order: the one builder of every forecast's outputs."""
        return _forecast_arrays(self.d, rows, fill, pit)

    def filter_forecasts(self, datas, interval: float = 0.975, keys=None):
        """cssm_fleet_filter_forecasts: ``ll_filter`` and, from the same launch, before every record is stepped, ``forecast`` of the
        record's time from the cloud before it (``ParticleFilter.getMeanForecast`` mapped over the filter stream).  ``keys``: per series
        an array of T_k Philox keys (None: the rule of ``forecast_key`` for every record).  ``(ll[S], [ll_t of series k], [ess_t of
        series k], fc, rc[S], fc_rc[S])``; ``fc`` is a list of S dicts with the nine statistic names of ``forecast`` plus ``obs_below``
        / ``obs_equal`` (the PIT counts: draws strictly below / equal to the datum; -1 without one), shapes [T_k, ...].  A row reads
        NaN behind the record at which the series failed, for a record whose time ``forecast`` refuses, and throughout a series whose
        ``fc_rc`` is not zero (a model without the scale its observation draw needs).  The fleet continues with ``step``."""
        if len(datas) != self.S:
            raise ValueError("one (t, y, has) triple per series")
        if keys is not None and len(keys) != self.S:
            raise ValueError("one array of keys per series")
        off, t, y, has = self.pack(datas, allow_empty=True)
        ky = None
        if keys is not None:
            o = [int(v) for v in off]
            per = [np.asarray([int(x) & (2**64 - 1) for x in np.asarray(v, dtype=object).ravel()], dtype=np.uint64) for v in keys]
            for k in range(self.S):
                if len(per[k]) != o[k + 1] - o[k]:
                    raise ValueError(f"series {k}: one key per record ({o[k + 1] - o[k]}), not {len(per[k])}")
            ky = np.ascontiguousarray(np.concatenate(per) if per else np.zeros(0), dtype=np.uint64)
        return self.filter_forecasts_packed(off, t, y, has, interval, ky)

    def filter_forecasts_packed(self, off, t, y, has, interval: float = 0.975, keys=None):
        """``filter_forecasts`` on arrays ``pack`` made and (optional) a uint64 array of off[-1] keys."""
        R, t, y, has = self._record_inputs(off, t, y, has)
        if keys is not None and (keys.dtype != np.uint64 or len(keys) != R or not keys.flags.c_contiguous):
            raise ValueError(f"keys must be a C-contiguous uint64 array of off[-1] = {R} entries")
        ll, rc, ll_t, ess_t = self._record_outputs(R)
        fc_rc = np.zeros(self.S, dtype=np.int32)
        arr, ptrs = self._forecast_arrays(R)
        self.generation += 1
        _abi.check(self.lib.cssm_fleet_filter_forecasts(self._h, _p(off), _p(t), _p(y), _p(has), _p(keys if R else None), float(interval), _p(ll),
                                                        _p(ll_t), _p(ess_t), *ptrs, _p(rc), _p(fc_rc)))
        return ll, self._split(off, ll_t), self._split(off, ess_t), self._split_named(off, arr), rc, fc_rc

    def step_forecast(self, t, y, has=None, active=None, keys=None, interval: float = 0.975):
        """cssm_fleet_step_forecast: ``step`` and, from the same launch, before the record is stepped, ``forecast`` of its time:
        ``(ll[S], ess[S], fc, rc[S], fc_rc[S])``; ``fc`` a dict of the nine statistics ([S, d] / [S]) and the PIT counts
        ``obs_below`` / ``obs_equal``; entries of series that are inactive, have no cloud or fail are NaN / -1.  ``keys``: S Philox
        keys (None: ``forecast_key(k)``)."""
        t, y, has, active = self._step_inputs(t, y, has, active)
        if keys is not None:
            if len(keys) != self.S:
                raise ValueError("one key per series")
            keys = np.ascontiguousarray([int(x) & (2**64 - 1) for x in keys], dtype=np.uint64)
        ll, ess, rc = self._step_outputs()
        fc_rc = np.zeros(self.S, dtype=np.int32)
        arr, ptrs = self._forecast_arrays(self.S)
        self.generation += 1
        _abi.check(self.lib.cssm_fleet_step_forecast(self._h, _p(active), _p(t), _p(y), _p(has), _p(keys), float(interval), _p(ll), _p(ess), *ptrs,
                                                     _p(rc), _p(fc_rc)))
        return ll, ess, arr, rc, fc_rc

    def interpolate(self, datas, interval: float = 0.975, reference_pairing: bool = False):
        """cssm_fleet_interpolate: ``NativePf.interpolate`` of every series in two launches.  ``(ll[S], per-series list of (mean[T_k + 1,
        d], lower, upper, eta_of_mean[T_k + 1], eta_lower, eta_upper), rc[S])``; rc[k] != 0 is series k's own status (-6: no records,
        -5: its weights were unusable) and its arrays and ll read NaN.  The fleet's clouds and clocks are not touched."""
        if len(datas) != self.S:
            raise ValueError("one (t, y, has) triple per series")
        return self.interpolate_packed(*self.pack(datas, allow_empty=True), interval=interval, reference_pairing=reference_pairing)

    def interpolate_packed(self, off, t, y, has, interval: float = 0.975, reference_pairing: bool = False):
        """``interpolate`` on arrays ``pack`` made (a caller that interpolates the same fleet repeatedly packs once)."""
        R, t, y, has = self._record_inputs(off, t, y, has)
        ll, rc = np.zeros(self.S), np.zeros(self.S, dtype=np.int32)
        rows = _interval_arrays((R + self.S,), self.d)
        _abi.check(self.lib.cssm_fleet_interpolate(self._h, _p(off), _p(t), _p(y), _p(has), float(interval),
                                                   _abi.CSSM_INTERP_REFERENCE_PAIRING if reference_pairing else 0, _p(ll), *map(_p, rows), _p(rc)))
        return ll, self.interpolate_rows(off, rows), rc

    @staticmethod
    def interpolate_rows(off, arrays):
        """Series k's rows of ``cssm_fleet_interpolate``'s outputs: ``off[k] + k .. off[k + 1] + k`` (T_k + 1 rows, row 0 the initial
        cloud) of every array, per series (``_split`` with a row more per series)."""
        per = [NativePfFleet._split(off, a, 1) for a in arrays]
        return [tuple(rows[k] for rows in per) for k in range(len(off) - 1)]

    def _ms(self, fn, count):
        """The ``count`` milliseconds one of the library's timing getters writes."""
        ms = np.zeros(count)
        _abi.check(fn(self._h, _p(ms)))
        return tuple(float(v) for v in ms)

    def interpolate_last_ms(self) -> Tuple[float, float]:
        """Device time (HIP events) of the last interpolation's forward launch and lineage launch, ms, summed over its chunks."""
        return self._ms(self.lib.cssm_fleet_interpolate_last_ms, 2)

    def smooth(self, datas, n_traj: Optional[int] = None, interval: float = 0.975, want_trajectories: bool = False):
        """cssm_fleet_smooth (an EXTENSION: the reference has no smoother beyond ``FilterInterpolate``): forward filtering, backward
        simulation of every series -- ``interpolate``'s forward pass, then ``n_traj`` trajectories (None: N) drawn backwards through the
        kept clouds and summarised per time index.  Returns what ``interpolate`` returns, ``(ll[S], per-series list of (mean[T_k + 1, d],
        lower, upper, eta_of_mean[T_k + 1], eta_lower, eta_upper), rc[S])``, and with ``want_trajectories`` a fourth entry: per series
        the uint32 array ``[T_k + 1, n_traj]`` of the particle of each kept cloud every trajectory passes through (0xffffffff throughout
        a series whose rc is not 0).  The fleet's clouds and clocks are not touched."""
        if len(datas) != self.S:
            raise ValueError("one (t, y, has) triple per series")
        return self.smooth_packed(*self.pack(datas, allow_empty=True), n_traj=n_traj, interval=interval, want_trajectories=want_trajectories)

    def smooth_packed(self, off, t, y, has, n_traj: Optional[int] = None, interval: float = 0.975, want_trajectories: bool = False):
        """``smooth`` on arrays ``pack`` made (a caller that smooths the same fleet repeatedly packs once)."""
        R, t, y, has = self._record_inputs(off, t, y, has)
        M = self.n if n_traj is None else int(n_traj)
        if not 1 <= M <= _abi.FLEET_MAX_N:
            raise ValueError(f"n_traj must be in [1, {_abi.FLEET_MAX_N}], not {M}")
        ll, rc = np.zeros(self.S), np.zeros(self.S, dtype=np.int32)
        rows = _interval_arrays((R + self.S,), self.d)
        traj = np.zeros((R + self.S, M), dtype=np.uint32) if want_trajectories else None
        _abi.check(self.lib.cssm_fleet_smooth(self._h, _p(off), _p(t), _p(y), _p(has), M, float(interval), 0, _p(ll), *map(_p, rows), _p(traj),
                                              _p(rc)))
        out = (ll, self.interpolate_rows(off, rows), rc)
        return out + (self._split(off, traj, 1),) if want_trajectories else out

    def smooth_last_ms(self) -> Tuple[float, float, float]:
        """Device time (HIP events) of the last ``smooth``'s forward launch, backward simulation and row summaries, ms, summed over its
        chunks."""
        return self._ms(self.lib.cssm_fleet_smooth_last_ms, 3)

    def if2(self, desc, datas, rw_sd, cooling: float, iters: int, seeds, theta0=None, swarm0=None, first_iter: int = 0, iters_per_launch: int = 0,
            want_swarm: bool = False, want_last: bool = False):
        """cssm_fleet_if2 (an EXTENSION: the reference has no likelihood maximiser): iterated filtering, a search per series from the rows
        of ``theta0[S, n_theta]`` (or the swarm ``swarm0[S, n_theta, N]`` of an earlier call, continued at ``first_iter``) under
        ``seeds``; ``desc`` is the descriptor the rows flatten, ``rw_sd[n_theta]`` the random-walk standard deviations, ``cooling`` the
        factor they shrink by over 50 iterations.  Returns a dict: ``theta_mean[S, iters, n_theta]``, ``ll[S, iters]``, ``rc[S]``; with
        ``want_swarm`` also ``swarm[S, n_theta, N]``; with ``want_last`` the last iteration's ``ll_t`` / ``ess_t`` (per series),
        ``x[S, d, N]`` and ``anc[S, N]``.  The fleet's clouds and clocks are not touched."""
        if len(datas) != self.S:
            raise ValueError("one (t, y, has) triple per series")
        off, t, y, has = self.pack(datas, allow_empty=True)
        R, t, y, has = self._record_inputs(off, t, y, has)
        if theta0 is None and swarm0 is None:
            raise ValueError("theta0 (a starting row per series) or swarm0 (a whole swarm) is needed")
        nt = self.n_theta
        th0 = None if theta0 is None else np.ascontiguousarray(theta0, dtype=np.float64).reshape(self.S, nt)
        sw0 = None if swarm0 is None else np.ascontiguousarray(swarm0, dtype=np.float64).reshape(self.S, nt, self.n)
        sd = np.ascontiguousarray(rw_sd, dtype=np.float64)
        if sd.shape != (nt,):
            raise ValueError(f"rw_sd must hold n_theta = {nt} standard deviations")
        keys = np.ascontiguousarray([int(x) & (2**64 - 1) for x in seeds], dtype=np.uint64)
        if len(keys) != self.S:
            raise ValueError("one seed per series")
        iters = int(iters)
        out = {"theta_mean": np.full((self.S, max(iters, 0), nt), np.nan), "ll": np.full((self.S, max(iters, 0)), np.nan),
               "rc": np.zeros(self.S, dtype=np.int32)}
        swarm = np.zeros((self.S, nt, self.n)) if want_swarm else None
        ll_t, ess_t = (np.zeros(max(R, 1)), np.zeros(max(R, 1), dtype=np.int32)) if want_last else (None, None)
        x, anc = (np.zeros((self.S, self.d, self.n)), np.zeros((self.S, self.n), dtype=np.uint32)) if want_last else (None, None)
        _abi.check(self.lib.cssm_fleet_if2(self._h, desc.ptr(), _p(th0), _p(sw0), nt, _p(sd), float(cooling), int(first_iter), iters,
                                           int(iters_per_launch), _p(keys), _p(off), _p(t), _p(y), _p(has), _p(out["theta_mean"]), _p(out["ll"]),
                                           _p(swarm), _p(ll_t), _p(ess_t), _p(x), _p(anc), _p(out["rc"])))
        if want_swarm:
            out["swarm"] = swarm
        if want_last:
            out.update(ll_t=self._split(off, ll_t[:R]), ess_t=self._split(off, ess_t[:R]), x=x, anc=anc)
        return out

    def if2_last_ms(self) -> float:
        """Device time (HIP events) of the launches of the last ``if2``, ms."""
        return self._ms(self.lib.cssm_fleet_if2_last_ms, 1)[0]

    def pmmh_last_split(self):
        """cssm_fleet_pmmh_last_split: milliseconds of the last ``cssm_fleet_pmmh_run`` on this fleet, summed over its iterations --
        (propose + set_params + reseed, record building, upload, kernel, decide) and the iterations counted."""
        ms = self._ms(self.lib.cssm_fleet_pmmh_last_split, 6)
        return ms[:5], int(ms[5])

    def pmmh_run(self, desc, theta0, delta, off, t, y, has, seeds, iters):
        """cssm_fleet_pmmh_run: a Metropolis chain per series from the rows of ``theta0[S, n_theta]`` under ``seeds``, ``desc`` the
        descriptor the rows flatten, on the arrays ``pack`` made: ``(ll[S, iters], theta[S, iters, n_theta], accepted[S, iters],
        last_state[S, iters, d])`` (``pmmh.pmmh_native_fleet`` is the caller's entry point)."""
        nt = theta0.shape[1]
        ll, th, last = np.zeros((self.S, iters)), np.zeros((self.S, iters, nt)), np.zeros((self.S, iters, self.d))
        acc = np.zeros((self.S, iters), dtype=np.int32)
        sd = np.ascontiguousarray([int(x) & (2**64 - 1) for x in seeds], dtype=np.uint64)
        self.generation += 1
        _abi.check(self.lib.cssm_fleet_pmmh_run(self._h, desc.ptr(), _p(theta0), nt, float(delta), _p(off), _p(t), _p(y), _p(has), _p(sd), int(iters),
                                                _p(ll), _p(th), _p(acc), _p(last)))
        return ll, th, acc, last

    def pmmh_chains(self, desc, theta0, chol, off, t, y, has, seeds, iters, priors=None, first_iter: int = 0, ll0=None, state0=None,
                    iters_per_launch: int = 0):
        """cssm_fleet_pmmh_chains: whole Metropolis chains on the device, a chain per series from the rows of ``theta0[S, n_theta]`` under
        ``seeds``, on the arrays ``pack`` made (``allow_empty``: a series without records is left alone, its rows read NaN).  ``chol``:
        the proposal's lower-triangular factor ``[n_theta, n_theta]``, or one per chain ``[S, n_theta, n_theta]``; ``priors``: None (all
        flat) or ``n_theta`` ``_abi.Prior`` entries (``pmmh.priors_for``); ``first_iter`` / ``ll0[S]`` / ``state0[S, d]`` continue chains.
        Returns ``(ll[S, iters], theta[S, iters, n_theta], accepted[S, iters], last_state[S, iters, d], diag[S, 2], rc[S])``.  The fleet's
        clouds, clocks, keys and parameters are not touched."""
        def data():
            return self._record_inputs(off, t, y, has)[1:]
        return self._chains_call(self.lib.cssm_fleet_pmmh_chains, desc, theta0, chol, seeds, iters, priors, first_iter, ll0, state0,
                                 iters_per_launch, off, data)

    def _chains_call(self, call, desc, theta0, chol, seeds, iters, priors, first_iter, ll0, state0, iters_per_launch, off, data):
        """What ``pmmh_chains`` and ``NativeLgcpFleet.pmmh_chains_lgcp`` share: the chains' inputs checked and laid out, ``call`` with
        ``off`` and the arrays ``data()`` returns (the packed records, checked, as that call takes them) between them and the outputs, and
        the six arrays they return."""
        nt = self.n_theta
        theta0 = np.ascontiguousarray(theta0, dtype=np.float64)
        if theta0.shape != (self.S, nt):
            raise ValueError(f"theta0 must be [S, n_theta] = [{self.S}, {nt}]")
        chol = np.ascontiguousarray(chol, dtype=np.float64)
        if chol.shape not in ((nt, nt), (self.S, nt, nt)):
            raise ValueError(f"chol must be [n_theta, n_theta] or [S, n_theta, n_theta] with n_theta = {nt}, S = {self.S}")
        pri = None
        if priors is not None:
            if len(priors) != nt:
                raise ValueError(f"priors must hold n_theta = {nt} entries")
            pri = (_abi.Prior * nt)(*priors)
        keys = np.ascontiguousarray([int(x) & (2**64 - 1) for x in seeds], dtype=np.uint64)
        if len(keys) != self.S:
            raise ValueError("one seed per chain")
        l0 = None if ll0 is None else np.ascontiguousarray(ll0, dtype=np.float64).reshape(self.S)
        s0 = None if state0 is None else np.ascontiguousarray(state0, dtype=np.float64).reshape(self.S, self.d)
        arrays = data()
        iters = int(iters)
        rows = max(iters, 0)
        ll, th, last = np.zeros((self.S, rows)), np.zeros((self.S, rows, nt)), np.zeros((self.S, rows, self.d))
        acc, diag, rc = np.zeros((self.S, rows), dtype=np.int32), np.zeros((self.S, 2), dtype=np.uint32), np.zeros(self.S, dtype=np.int32)
        _abi.check(call(self._h, desc.ptr(), _p(theta0), nt, _p(chol), int(chol.ndim == 3), pri, _p(l0), _p(s0), int(first_iter), iters,
                        int(iters_per_launch), _p(keys), _p(off), *[_p(a) for a in arrays], _p(ll), _p(th), _p(acc), _p(last), _p(diag),
                        _p(rc)))
        return ll, th, acc, last, diag, rc

    def pmmh_chains_last_ms(self) -> float:
        """Device time (HIP events) of the launches of the last ``pmmh_chains``, ms."""
        return self._ms(self.lib.cssm_fleet_pmmh_chains_last_ms, 1)[0]

    def init(self, t0):
        t0 = np.ascontiguousarray(np.broadcast_to(np.asarray(t0, dtype=np.float64), (self.S,)), dtype=np.float64)
        self.generation += 1
        _abi.check(self.lib.cssm_fleet_init(self._h, _p(t0)))

    def pack_states(self, rows):
        """The ragged states of ``cssm_fleet_init_from`` from a sequence of S arrays ``[M_k, d]`` or ``[d]`` (None or empty: M_k = 0):
        ``(moff uint64[S + 1], x float64[M, d])``, C-contiguous -- ``pack_posteriors`` without the parameter rows."""
        if len(rows) != self.S:
            raise ValueError("one array of states per series (None or empty: none)")
        post = []
        for k, r in enumerate(rows):
            x = np.zeros(0) if r is None else np.asarray(r, dtype=np.float64)
            if x.size % self.d:
                raise ValueError(f"series {k}: its states hold {x.size} numbers, no multiple of d = {self.d}")
            x = x.reshape(-1, self.d)
            post.append((np.zeros((len(x), 1)), x) if len(x) else None)      # (rows of one placeholder parameter: not handed on)
        moff, _, x = self.pack_posteriors(post, n_theta=1)
        return moff, x

    def init_from(self, t0s, rows, picks=None, keys=None, active=None):
        """cssm_fleet_init_from: the clouds of the active series (``active`` None = all) come from the caller.  ``rows[k]``: ``[d]`` or
        ``[1, d]`` -- that state replicated, ``FilterInit`` -- or ``[M_k, d]``, a posterior sample of the state at ``t0s[k]`` (a scalar serves
        every series); particle i of series k then starts at row ``picks[k, i]`` (``picks``: [S, N] indices, series k's below M_k) or, without
        ``picks``, at the row ``cssm_fleet_forecast_posterior`` selects under ``keys[k]`` (S Philox keys).  ``(pick_out uint32[S, N], rc[S])``;
        rc[k] != 0 is series k's own refusal (-6: no rows, a non-finite t0 or entry, a pick out of range, M_k > 1 with neither picks nor
        keys), the series is then left as it was and its picks read 0.  The series continue with ``step`` or ``ll_filter_more``."""
        moff, x = self.pack_states(rows)
        t0 = np.asarray(t0s, dtype=np.float64)
        if t0.ndim != 0 and t0.shape != (self.S,):
            raise ValueError("one t0 per series (or one for all)")
        t0 = np.ascontiguousarray(np.broadcast_to(t0, (self.S,)), dtype=np.float64)
        pk = None
        if picks is not None:
            pa = np.asarray(picks)
            if pa.shape != (self.S, self.n) or (pa < 0).any():
                raise ValueError(f"picks must hold S x N = {self.S} x {self.n} non-negative indices")
            pk = np.ascontiguousarray(pa, dtype=np.uint32)
        ky = None
        if keys is not None:
            if len(keys) != self.S:
                raise ValueError("one key per series")
            ky = np.ascontiguousarray([int(v) & (2**64 - 1) for v in keys], dtype=np.uint64)
        xx = x if len(x) else np.zeros((1, self.d))
        pick_out = np.zeros((self.S, self.n), dtype=np.uint32)
        rc = np.zeros(self.S, dtype=np.int32)
        self.generation += 1
        _abi.check(self.lib.cssm_fleet_init_from(self._h, _p(_u8(active)), _p(t0), _p(moff), _p(xx), _p(pk), _p(ky), _p(pick_out), _p(rc)))
        return pick_out, rc

    def copy_series(self, map, src: Optional["NativePfFleet"] = None, keys: bool = False):
        """cssm_fleet_copy_series (EXTENSION): series k <- series ``map[k]`` of ``src`` (None = this fleet), simultaneously and on the
        device -- cloud, ancestors, ll / ess, clock, observation index, parameters; with ``keys`` the Philox key too (by default series k
        keeps its own).  ``map``: S integers, -1 or None = keep.  ``rc[S]``: -7 where the source series has no cloud (series k is then
        left as it was)."""
        if len(map) != self.S:
            raise ValueError(f"one map entry per series ({self.S}), not {len(map)}")
        mp = np.ascontiguousarray([_abi.CSSM_FLEET_COPY_KEEP if v is None else int(v) for v in map], dtype=np.int64)
        other = self if src is None else src
        rc = np.zeros(self.S, dtype=np.int32)
        self.generation += 1
        _abi.check(self.lib.cssm_fleet_copy_series(self._h, other._h, _p(mp.view(np.uint64)), _abi.CSSM_FLEET_COPY_KEYS if keys else 0, _p(rc)))
        if keys:   # (forecast_key reads them)
            old = list(other.seeds)
            for k in range(self.S):
                if mp[k] >= 0 and rc[k] == 0:
                    self.seeds[k] = old[int(mp[k])]
        return rc

    def _step_inputs(self, t, y, has, active):
        """What every step call starts with: ``(t, y, has, active)`` as the C call takes them (None stays None), one ``(t, y)`` per
        series or a refusal.  The caller holds them across its C call."""
        t = np.ascontiguousarray(t, dtype=np.float64); y = np.ascontiguousarray(y, dtype=np.float64)
        if len(t) != self.S or len(y) != self.S:
            raise ValueError("one (t, y) per series")
        return t, y, _u8(has), _u8(active)

    def _step_outputs(self):
        """``(ll[S], ess[S], rc[S])`` of a step call, preset to NaN / -1 / 0: what the entries of a series it does not move read."""
        return np.full(self.S, np.nan), np.full(self.S, -1, dtype=np.int32), np.zeros(self.S, dtype=np.int32)

    def step(self, t, y, has=None, active=None):
        """One observation for the active series (``active`` None = all): ``(ll[S], ess[S], rc[S])``; entries of inactive series are
        NaN / -1 / 0."""
        t, y, has, active = self._step_inputs(t, y, has, active)
        ll, ess, rc = self._step_outputs()
        self.generation += 1
        _abi.check(self.lib.cssm_fleet_step(self._h, _p(active), _p(t), _p(y), _p(has), _p(ll), _p(ess), _p(rc)))
        return ll, ess, rc

    def step_intervals(self, t, y, has=None, active=None, interval: float = 0.975):
        """cssm_fleet_step_intervals: ``step`` and, from the same launch, ``summary`` of every cloud it moved: ``(ll[S], ess[S], (state_mean[S,
        d], state_lower, state_upper, eta_of_mean[S], eta_lower, eta_upper), rc[S])``; entries of series that are inactive, have no cloud
        or fail are NaN / -1."""
        t, y, has, active = self._step_inputs(t, y, has, active)
        ll, ess, rc = self._step_outputs()
        rows = _interval_arrays((self.S,), self.d, np.nan)
        self.generation += 1
        _abi.check(self.lib.cssm_fleet_step_intervals(self._h, _p(active), _p(t), _p(y), _p(has), float(interval), _p(ll), _p(ess), *map(_p, rows),
                                                      _p(rc)))
        return ll, ess, rows, rc

    def window(self, slices: int):
        """cssm_fleet_window: remember, per series, the ``slices`` most recent clouds and ancestor arrays on the device (S x slices x N
        x (8 d + 4) bytes) for ``step_interpolate``; 0 frees them.  Every window restarts."""
        if int(slices) < 0:
            raise ValueError("slices must not be negative")
        _abi.check(self.lib.cssm_fleet_window(self._h, int(slices)))

    def window_depth(self, k: int) -> int:
        """The records remembered behind series k's base slice (cssm_fleet_window_depth): 0 .. slices - 1."""
        return int(self.lib.cssm_fleet_window_depth(self._h, int(k)))

    def _lags(self, lag, max_lag: int):
        """``step_interpolate``'s ``lag`` as the C call takes it: None (every series max_lag), or uint32[S] with CSSM_FLEET_NO_ROWS where
        an entry is None (a C-contiguous uint32 array is taken as it is).  Refused here, before any device call: a negative max_lag, a sequence of another length than S, a negative
        entry."""
        if int(max_lag) < 0 or int(max_lag) >= _abi.CSSM_FLEET_NO_ROWS:
            raise ValueError("max_lag must be in 0 .. 2^32 - 2")
        if lag is None:
            return None
        if np.ndim(lag) == 0:
            lag = [lag] * self.S
        if len(lag) != self.S:
            raise ValueError(f"one lag per series ({self.S}), not {len(lag)}")
        if isinstance(lag, np.ndarray) and lag.dtype == np.uint32 and lag.flags.c_contiguous:
            return lag                                  # (as the C call takes it: a caller that streams builds it once)
        if any(v is not None and int(v) < 0 for v in lag):
            raise ValueError("a lag must not be negative (None asks for no rows)")
        return np.ascontiguousarray([_abi.CSSM_FLEET_NO_ROWS if v is None else int(v) for v in lag], dtype=np.uint32)

    def step_interpolate(self, t, y, has=None, active=None, lag=None, max_lag: int = 0, interval: float = 0.975):
        """cssm_fleet_step_interpolate: ``step``, which also remembers every cloud it moved in the series' window, and (a second launch)
        the fixed-lag interpolation of the series that ask: ``(ll[S], ess[S], rows_out[S], (state_mean[S, max_lag + 1, d], state_lower,
        state_upper, eta_of_mean[S, max_lag + 1], eta_lower, eta_upper), rc[S])``.  Row j of series k summarises time index (newest - j)
        through the lineages that survive to the cloud just written; ``rows_out[k]`` = min(lag_k, window_depth(k)) + 1 rows are filled,
        the others read NaN.  ``lag``: None (max_lag for every series), an int, or one entry per series with None for "no rows"."""
        t, y, has, active = self._step_inputs(t, y, has, active)
        lag = self._lags(lag, max_lag)
        ll, ess, rc = self._step_outputs()
        nrows = np.zeros(self.S, dtype=np.uint32)
        rows = _interval_arrays((self.S, int(max_lag) + 1), self.d, np.nan)
        self.generation += 1
        _abi.check(self.lib.cssm_fleet_step_interpolate(self._h, _p(active), _p(t), _p(y), _p(has), _p(lag), int(max_lag), float(interval), _p(ll),
                                                        _p(ess), _p(nrows), *map(_p, rows), _p(rc)))
        return ll, ess, nrows, rows, rc

    def step_interpolate_last_ms(self) -> Tuple[float, float]:
        """Device time (HIP events) of the last ``step_interpolate``'s forward launch and lineage launch, ms (the latter 0 when no
        series asked for rows)."""
        return self._ms(self.lib.cssm_fleet_step_interpolate_last_ms, 2)

    def summary(self, interval: float = 0.975):
        """(state_mean[S, d], state_lower[S, d], state_upper[S, d], eta_of_mean[S], eta_lower[S], eta_upper[S])."""
        rows = _interval_arrays((self.S,), self.d)
        _abi.check(self.lib.cssm_fleet_summary(self._h, float(interval), *map(_p, rows)))
        return rows

    def particles(self, k: int) -> np.ndarray:
        out = np.zeros((self.d, self.n))
        _abi.check(self.lib.cssm_fleet_get_particles(self._h, int(k), _p(out)))
        return out

    def ancestors(self, k: int) -> np.ndarray:
        out = np.zeros(self.n, dtype=np.uint32)
        _abi.check(self.lib.cssm_fleet_get_ancestors(self._h, int(k), _p(out)))
        return out

    def last_ms(self) -> Tuple[float, float, float]:
        """Device time (HIP events) of the last ll_filter / init / step call, of the last summary and of the last forecast, ms;
        < 0: none yet."""
        return self._ms(self.lib.cssm_fleet_last_ms, 3)

    def observation_index(self, k: int) -> int:
        """Observations series k's current cloud has seen (cssm_fleet_observation_index)."""
        return int(self.lib.cssm_fleet_observation_index(self._h, int(k)))

    def forecast_key(self, k: int) -> int:
        """The default Philox key of a forecast of series k's current cloud: cssm_pf_run_key(seed_k, 2^63 | observation index), the
        rule of ``NativePf.forecast_key``."""
        return int(self.lib.cssm_pf_run_key(self.seeds[k], (1 << 63) | self.observation_index(k)))

    def pack_times(self, times):
        """The ragged arrays of ``cssm_fleet_forecast`` from a sequence of S arrays of future times (None or empty: no horizons for
        that series): ``(off uint64[S + 1], t float64)``, C-contiguous.  A wrong number of series is refused here."""
        if len(times) != self.S:
            raise ValueError("one array of times per series (None or empty: none)")
        ts = [np.zeros(0) if v is None else np.asarray(v, dtype=np.float64).ravel() for v in times]
        off = np.zeros(self.S + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(v) for v in ts], dtype=np.uint64)
        t = np.ascontiguousarray(np.concatenate(ts) if ts else np.zeros(0), dtype=np.float64)
        return off, t

    def forecast(self, times, keys=None, interval: float = 0.975, want_samples: bool = False):
        """cssm_fleet_forecast: every series' horizons in one launch.  ``times``: S arrays (None / empty: none for that series);
        ``keys``: S Philox keys (None: ``forecast_key(k)``).  A list of S dicts with the keys of ``NativePf.forecast`` and shapes
        [H_k, ...], plus ``rc``, the series' own status (its arrays read NaN when it is not zero).  The fleet is not touched."""
        off, t = self.pack_times(times)
        if keys is None:
            keys = [self.forecast_key(k) for k in range(self.S)]
        if len(keys) != self.S:
            raise ValueError("one key per series")
        ky = np.ascontiguousarray([int(x) & (2**64 - 1) for x in keys], dtype=np.uint64)
        arr, samples, rc = self.forecast_packed(off, t, ky, interval, want_samples)
        return self._forecast_dicts(off, arr, samples, ky, rc)

    def _forecast_dicts(self, off, arr, samples, keys, rc):
        """Per series what a forecast returns: its rows of the nine statistics and of the samples (None without them), its key and its
        status."""
        outs = self._split_named(off, arr)
        per = [None] * self.S if samples is None else self._split(off, samples)
        for k, r in enumerate(outs):
            r["samples"] = per[k]; r["key"] = int(keys[k]); r["rc"] = int(rc[k])
        return outs

    def forecast_packed(self, off, t, keys, interval: float = 0.975, want_samples: bool = False):
        """``forecast`` on the arrays ``pack_times`` made and a uint64 array of keys (a caller that forecasts the same fleet repeatedly
        packs once): ``(dict of arrays laid out like t, samples or None, rc[S])``."""
        R = int(off[-1])
        tt = t if R else np.zeros(1)
        arr, ptrs = self._forecast_arrays(R, 0.0, pit=False)
        samples = np.zeros((R, self.d + 3, self.n)) if want_samples else None
        rc = np.zeros(self.S, dtype=np.int32)
        _abi.check(self.lib.cssm_fleet_forecast(self._h, _p(off), _p(tt), _p(keys), float(interval), *ptrs, _p(samples), _p(rc)))
        return arr, samples, rc

    def simulate(self, t0s, times, n_paths: int = 1, keys=None):
        """cssm_fleet_simulate: every series drawn from its own model (the parameters of ``set_params``) in one launch per chunk.
        ``t0s``: S start times (a scalar serves every series); ``times``: S arrays (None / empty: the row at t0 alone); ``keys``: S
        Philox keys (None: ``simulate.fleet_keys(self.seeds)`` = cssm_pf_run_key(seed_k, 2^62 | k)).  ``([rows of series k: [T_k + 1,
        d + 3, n_paths]], rc[S])`` -- per series what ``simulate.simulate`` returns under its model, key and times; the rows of a
        series whose rc is not zero read NaN.  The fleet is not touched and no series needs a cloud."""
        off, t = self.pack_times(times)
        t0 = np.asarray(t0s, dtype=np.float64)
        if t0.ndim != 0 and t0.shape != (self.S,):
            raise ValueError("one t0 per series (or one for all)")
        t0 = np.ascontiguousarray(np.broadcast_to(t0, (self.S,)), dtype=np.float64)
        if keys is None:
            from .simulate import fleet_keys
            keys = fleet_keys(self.seeds)
        if len(keys) != self.S:
            raise ValueError("one key per series")
        ky = np.ascontiguousarray([int(x) & (2**64 - 1) for x in keys], dtype=np.uint64)
        out, rc = self.simulate_packed(t0, off, t, ky, n_paths)
        return self._split(off, out, 1), rc

    def simulate_packed(self, t0, off, t, keys, n_paths: int = 1):
        """``simulate`` on float64 t0[S], the arrays ``pack_times`` made and uint64 keys[S]: ``(rows [off[-1] + S, d + 3, n_paths], rc[S])``,
        series k's rows at ``off[k] + k .. off[k + 1] + k``."""
        R = int(off[-1])
        tt = t if R else np.zeros(1)
        out = np.zeros((R + self.S, self.d + 3, int(n_paths)))
        rc = np.zeros(self.S, dtype=np.int32)
        _abi.check(self.lib.cssm_fleet_simulate(self._h, int(n_paths), _p(t0), _p(off), _p(tt), _p(keys), _p(out), _p(rc)))
        return out, rc

    def simulate_last_ms(self) -> float:
        """Device time (ms: upload, kernels, read-back) of the last ``simulate``."""
        return self._ms(self.lib.cssm_fleet_simulate_last_ms, 1)[0]

    def posterior_key(self, k: int) -> int:
        """The default Philox key of series k's posterior forecast: cssm_pf_run_key(seed_k, 2^63) -- ``forecast_key()`` of a fresh
        ``NativePf`` with that seed, the handle ``ParticleFilter.forecastPosterior`` makes."""
        return int(self.lib.cssm_pf_run_key(self.seeds[k], 1 << 63))

    def pack_posteriors(self, posteriors, n_theta: Optional[int] = None):
        """The ragged posteriors of ``cssm_fleet_forecast_posterior`` from a sequence of S ``(theta[M_k, n_theta], x[M_k, d])`` pairs
        (None or empty arrays: M_k = 0): ``(moff uint64[S + 1], theta float64[M, n_theta], x float64[M, d])``, C-contiguous.  A wrong
        number of series, rows of differing length and states of another dimension are refused here.  ``n_theta``: the length of a
        row; None: the descriptor's (``self.n_theta``), or what the first row tells where the fleet has no descriptor."""
        if len(posteriors) != self.S:
            raise ValueError("one (theta, x) posterior per series (None or empty: none)")
        if n_theta is None:
            n_theta = getattr(self, "n_theta", None)
        ths, xs = [], []
        for k, p in enumerate(posteriors):
            th = None if p is None else np.asarray(p[0], dtype=np.float64)
            if th is None or th.size == 0:
                ths.append(None); xs.append(None)
                continue
            th = np.atleast_2d(th)
            x = np.asarray(p[1], dtype=np.float64).reshape(th.shape[0], -1)
            if th.ndim != 2 or x.shape != (th.shape[0], self.d):
                raise ValueError(f"series {k}: theta must be M x n_theta and x M x d = {th.shape[0]} x {self.d} (got {th.shape}, {x.shape})")
            if n_theta is None:
                n_theta = th.shape[1]
            if th.shape[1] != n_theta:
                raise ValueError(f"series {k}: its rows hold {th.shape[1]} parameters, the others {n_theta}")
            ths.append(th); xs.append(x)
        nt = int(n_theta or 0)
        moff = np.zeros(self.S + 1, dtype=np.uint64)
        moff[1:] = np.cumsum([0 if v is None else len(v) for v in ths], dtype=np.uint64)
        theta = np.ascontiguousarray(np.concatenate([np.zeros((0, nt))] + [v for v in ths if v is not None]), dtype=np.float64)
        x = np.ascontiguousarray(np.concatenate([np.zeros((0, self.d))] + [v for v in xs if v is not None]), dtype=np.float64)
        return moff, theta, x

    def forecast_posterior(self, posteriors, t0s, times, keys=None, interval: float = 0.975, picks=None, want_samples: bool = False):
        """cssm_fleet_forecast_posterior: every series' posterior-predictive forecast in one launch.  ``posteriors[k]`` =
        ``(theta[M_k, n_theta], x[M_k, d])``, series k's joint posterior sample, its states at ``t0s[k]`` (a scalar serves every
        series); ``times``: S arrays (None / empty: none for that series); ``keys``: S Philox keys (None: ``posterior_key(k)``);
        ``picks``: None (drawn under the keys) or [S, N] indices, series k's below M_k.  A list of S dicts with the keys of
        ``forecast`` plus ``pick`` (uint32[N]): per series what ``NativePf.forecast_posterior`` returns on a handle of N particles.
        The fleet lends its structure and scratch only: no series needs a cloud, none is touched."""
        moff, theta, x = self.pack_posteriors(posteriors)
        t0 = np.asarray(t0s, dtype=np.float64)
        if t0.ndim != 0 and t0.shape != (self.S,):
            raise ValueError("one t0 per series (or one for all)")
        t0 = np.ascontiguousarray(np.broadcast_to(t0, (self.S,)), dtype=np.float64)
        off, t = self.pack_times(times)
        if keys is not None and len(keys) != self.S:
            raise ValueError("one key per series")
        pk = None
        if picks is not None:
            pa = np.asarray(picks)
            if pa.shape != (self.S, self.n) or (pa < 0).any():
                raise ValueError(f"picks must hold S x N = {self.S} x {self.n} non-negative indices")
            pk = np.ascontiguousarray(pa, dtype=np.uint32)
        if keys is None:
            keys = [self.posterior_key(k) for k in range(self.S)]
        ky = np.ascontiguousarray([int(v) & (2**64 - 1) for v in keys], dtype=np.uint64)
        arr, samples, pick_out, rc = self.forecast_posterior_packed(moff, theta, x, t0, off, t, ky, interval, pk, want_samples)
        outs = self._forecast_dicts(off, arr, samples, ky, rc)
        for k, r in enumerate(outs):
            r["pick"] = pick_out[k]
        return outs

    def forecast_posterior_packed(self, moff, theta, x, t0, off, t, keys, interval: float = 0.975, picks=None, want_samples: bool = False):
        """``forecast_posterior`` on the arrays ``pack_posteriors`` and ``pack_times`` made, float64 t0[S], uint64 keys[S] and (optional)
        uint32 picks[S, N]: ``(dict of arrays laid out like t, samples or None, pick uint32[S, N], rc[S])``."""
        R, M = int(off[-1]), int(moff[-1])
        tt = t if R else np.zeros(1)
        th = theta if M else np.zeros((1, max(1, theta.shape[1])))
        xx = x if M else np.zeros((1, self.d))
        arr, ptrs = self._forecast_arrays(R, 0.0, pit=False)
        samples = np.zeros((R, self.d + 3, self.n)) if want_samples else None
        pick_out = np.zeros((self.S, self.n), dtype=np.uint32)
        rc = np.zeros(self.S, dtype=np.int32)
        _abi.check(self.lib.cssm_fleet_forecast_posterior(self._h, self._desc.ptr(), _p(moff), _p(th), int(theta.shape[1]), _p(xx), _p(t0), _p(off),
                                                          _p(tt), _p(picks), _p(keys), float(interval), *ptrs, _p(samples), _p(pick_out), _p(rc)))
        return arr, samples, pick_out, rc


class NativeLgcpFleet(NativePfFleet):
    """``cssm_fleet*`` made by ``cssm_fleet_create_lgcp``: S event streams of a log-Gaussian Cox process filtered per launch, each as
    ``FilterLgcp(model, resample, precision)`` filters it on a handle of its own.  Every record is an event: ``y`` and ``has`` are
    ignored.  The calls an LGCP fleet does not serve (intervals and forecasts per record, interpolation, simulation, ``pmmh_run`` and
    ``pmmh_chains``) raise with the library's refusal; ``pmmh_chains_lgcp`` runs whole PMMH chains over its event streams."""

    _CREATE = "cssm_fleet_create_lgcp"

    def __init__(self, model: Model, n: int, series: int, precision: int, device: int = 0):
        self.precision = int(precision)
        super().__init__(model, n, series, device)

    def _descriptor(self, model: Model):
        return model.descriptor(self.precision)

    @staticmethod
    def pack(datas, allow_empty: bool = False):
        """``NativePfFleet.pack`` that also takes a bare array of event times per series (``simulate.lgcp_fleet_data``) in place of a
        ``(t, y, has)`` triple: its y reads 1.0 and its has 1, as ``lgcp_events_data`` writes them -- the library reads neither."""
        def triple(tr):
            if isinstance(tr, (tuple, list)) and len(tr) in (2, 3) and np.ndim(tr[0]) == 1:
                return tr
            t = np.asarray(tr, dtype=np.float64).ravel()
            return t, np.ones(len(t)), None
        return NativePfFleet.pack([triple(tr) for tr in datas], allow_empty)

    def pmmh_chains_lgcp(self, desc, theta0, chol, off, t, seeds, iters, priors=None, first_iter: int = 0, ll0=None, state0=None,
                         iters_per_launch: int = 0):
        """cssm_fleet_pmmh_chains_lgcp: ``NativePfFleet.pmmh_chains`` for event streams -- whole Metropolis chains on the device, a chain
        per stream from the rows of ``theta0[S, n_theta]`` under ``seeds``, on the ``off`` and ``t`` that ``pack`` made (every record is
        an event: no ``y``, no ``has``; ``allow_empty``: a stream without events is left alone, its rows read NaN).  ``desc``: an LGCP
        descriptor of the fleet's structure and precision.  ``chol``, ``priors``, ``first_iter`` / ``ll0`` / ``state0`` and
        ``iters_per_launch`` (0 = all iterations in one launch) as there.  Returns ``(ll[S, iters], theta[S, iters, n_theta],
        accepted[S, iters], last_state[S, iters, d], diag[S, 2], rc[S])``.  The fleet's clouds, clocks, keys, parameters and predicted
        levels are not touched."""
        def data():
            R = int(off[-1]) if isinstance(off, np.ndarray) and off.ndim == 1 and len(off) else 0
            self._check_packed(off, t, np.zeros(R), np.zeros(R, dtype=np.uint8))
            return (t if R else np.zeros(1),)
        return self._chains_call(self.lib.cssm_fleet_pmmh_chains_lgcp, desc, theta0, chol, seeds, iters, priors, first_iter, ll0, state0,
                                 iters_per_launch, off, data)

    def pmmh_chains_lgcp_last_ms(self) -> float:
        """Device time (HIP events) of the launches of the last ``pmmh_chains_lgcp``, ms."""
        return self._ms(self.lib.cssm_fleet_pmmh_chains_lgcp_last_ms, 1)[0]


class _PfView(NativePf):
    """A chain of a batch seen as a NativePf: the batch owns the handle, closing the view destroys nothing."""

    def close(self):
        self._h = C.c_void_p()

    __del__ = close


class Resampling:
    """``Resampling.systematicResampling`` (Resampling.scala:63-72) on the GPU.

    Called as a function it is the ``Resample[A]`` of package.scala:23: ``(samples, weights) ->
    samples`` where ``weights`` are the unnormalised ``w1 = exp(w - max)`` (ParticleFilter.scala:
    125-126).  Passed to ``Filter`` it only selects the native resampler -- the cloud never
    leaves the device.
    """

    @staticmethod
    def indentity(samples: Sequence, weights: Sequence[float]):
        """Resampling.indentity (sic), model/Resampling.scala:29: the samples as they are."""
        return samples

    @staticmethod
    def systematicAncestors(weights: Sequence[float], u: float, device: int = 0) -> np.ndarray:
        w = np.ascontiguousarray(weights, dtype=np.float64)
        anc = np.zeros(len(w), dtype=np.uint32)
        _abi.check(_abi.load_library().cssm_resample_systematic(_p(w), len(w), float(u), _p(anc), device))
        return anc

    @staticmethod
    def ancestors(kind: int, weights: Sequence[float], u: float = 0.0, seed: int = 0, step: int = 0, device: int = 0) -> np.ndarray:
        """cssm_resample: the ancestor indices of resampler ``kind`` (0 systematic, 1 stratified, 2 multinomial)."""
        w = np.ascontiguousarray(weights, dtype=np.float64)
        anc = np.zeros(len(w), dtype=np.uint32)
        _abi.check(_abi.load_library().cssm_resample(int(kind), _p(w), len(w), float(u), int(seed), int(step),
                                                     _p(anc), device))
        return anc

    @staticmethod
    def _seeded(kind: int, particles: Sequence, weights: Sequence[float], seed: Optional[int], step: int):
        if len(particles) != len(weights):
            raise ValueError("particles and weights differ in length")
        if seed is None:   # the reference draws from unseeded global generators (:83, :93)
            seed = int(np.random.default_rng().integers(0, 2**63))
        return [particles[int(a)] for a in Resampling.ancestors(kind, weights, 0.0, seed, step)]

    @staticmethod
    def stratifiedResampling(particles: Sequence, weights: Sequence[float], seed: Optional[int] = None, step: int = 0):
        """Resampling.scala:78-86 as a ``Resample[A]``; as a ``Filter`` argument it selects the native stratified resampler."""
        return Resampling._seeded(1, particles, weights, seed, step)

    @staticmethod
    def multinomialResampling(particles: Sequence, weights: Sequence[float], seed: Optional[int] = None, step: int = 0):
        """Resampling.scala:92-96 as a ``Resample[A]``; as a ``Filter`` argument it selects the native multinomial resampler."""
        return Resampling._seeded(2, particles, weights, seed, step)

    @staticmethod
    def residualAncestors(weights: Sequence[float], seed: int = 0, step: int = 0, device: int = 0) -> np.ndarray:
        """cssm_resample_residual (an EXTENSION, see ``residualResampling``): the particle every slot takes."""
        w = np.ascontiguousarray(weights, dtype=np.float64)
        anc = np.zeros(len(w), dtype=np.uint32)
        _abi.check(_abi.load_library().cssm_resample_residual(_p(w), len(w), int(seed), int(step), _p(anc), device))
        return anc

    @staticmethod
    def residualResampling(particles: Sequence, weights: Sequence[float], seed: Optional[int] = None, step: int = 0):
        """EXTENSION.  The reference's residualResampling (Resampling.scala:130-146) cannot run as written: it hands ``Vector.range(1, m)``
        with n weights to the multinomial resampler, indexes the particles with the result (:144-145) and exp-normalises weights that
        are already exponentiated.  This is the resampler its scaladoc DESCRIBES (:124-129), as a host ``Resample[A]``: particle i
        appears floor(n w_i / sum w) times, the remaining slots are drawn by multinomial resampling on the residual weights
        (cssm_resample_residual).  ``weights`` are w1 = exp(w - max), as for the other resamplers.  As a ``Filter`` argument it runs
        through the host-resampler seam (cssm_pf_propagate / cssm_pf_adopt): there is no native in-filter kernel for it; the filter
        keys its draws by (the filter's seed, the number of observations it has resampled), so a seeded Filter reproduces.  Called
        directly with seed = None it takes a fresh seed, as the reference's unseeded generators would."""
        if len(particles) != len(weights):
            raise ValueError("particles and weights differ in length")
        if seed is None:
            seed = int(np.random.default_rng().integers(0, 2**63))
        return [particles[int(a)] for a in Resampling.residualAncestors(weights, seed, step)]

    @staticmethod
    def systematicResampling(particles: Sequence, weights: Sequence[float], u: Optional[float] = None):
        if len(particles) != len(weights):
            raise ValueError("particles and weights differ in length")
        if u is None:  # the reference draws from the unseeded global scala.util.Random (:66)
            u = float(np.random.default_rng().random())
        anc = Resampling.systematicAncestors(weights, u)
        return [particles[int(a)] for a in anc]


# --------------------------------------------------------------------------- PfState
@dataclass(frozen=True)
class PfState:  # ParticleFilter.scala:32-37
    t: float
    observation: Optional[float]
    ll: float
    ess: int
    _owner: Optional[NativePf] = field(default=None, repr=False, compare=False)
    _generation: int = field(default=-1, repr=False, compare=False)

    @property
    def particles(self) -> np.ndarray:
        """The resampled cloud, SoA ``[d, N]`` (row k = component k in Tree.flatten order)."""
        if self._owner is None or self._owner.generation != self._generation:
            raise RuntimeError("this PfState is not the handle's current state; its cloud was advanced on the device")
        return self._owner.particles()


@dataclass(frozen=True)
class CredibleInterval:  # ParticleFilter.scala:14
    lower: float
    upper: float


@dataclass(frozen=True)
class PfOut:  # ParticleFilter.scala:20-26
    time: float
    observation: Optional[float]
    eta: float
    etaIntervals: CredibleInterval
    state: np.ndarray
    stateIntervals: List[CredibleInterval]


@dataclass(frozen=True)
class ForecastOut:  # ParticleFilter.scala:71-78
    t: float
    obs: float
    obsIntervals: CredibleInterval
    eta: float
    etaIntervals: CredibleInterval
    state: np.ndarray
    stateIntervals: List[CredibleInterval]


@dataclass(frozen=True)
class ObservationWithState:  # ParticleFilter.scala:381-382, one per particle there; here struct-of-arrays over the N particles
    t: float
    observation: np.ndarray   # [N]
    eta: np.ndarray           # [N]
    gamma: np.ndarray         # [N]
    sdeState: np.ndarray      # [d, N]


@dataclass(frozen=True)
class StateSpace:  # Sde.scala:170
    time: float
    state: np.ndarray


def _pfout_of(t, observation, row) -> PfOut:
    """One ``PfOut`` from the six values of a summary, in ``NativePf.summary``'s order."""
    m, lo, hi, em, el, eu = row
    return PfOut(float(t), observation, float(em), CredibleInterval(float(el), float(eu)), np.array(m, dtype=np.float64),
                 [CredibleInterval(float(a), float(b)) for a, b in zip(lo, hi)])


def pfouts_from_rows(times, observations, rows) -> List[PfOut]:
    """The ``PfOut`` of every row of ``NativePf.filter_intervals``' six arrays (state_mean[R, d], state_lower, state_upper, eta_of_mean[R],
    eta_lower, eta_upper), with the rows' times and observations."""
    m, lo, hi, em, el, eu = rows
    if not (len(times) == len(observations) == len(m) == len(lo) == len(hi) == len(em) == len(el) == len(eu)):
        raise ValueError("times, observations and the six row arrays must have one entry per row")
    return [_pfout_of(times[r], observations[r], (m[r], lo[r], hi[r], em[r], el[r], eu[r])) for r in range(len(times))]


# --------------------------------------------------------------------------- filters
class _FilterBase:
    lgcp_precision = 0

    def __init__(self, mod: Model, resample, n_particles: Optional[int] = None, seed: int = 20260101, device: int = 0):
        kinds = {Resampling.systematicResampling: 0, Resampling.stratifiedResampling: 1, Resampling.multinomialResampling: 2}
        if not callable(resample):
            raise TypeError("resample must be a Resample[A]: (samples, weights) -> samples")
        # one of the three native resamplers: the whole step stays on the device.  Any OTHER function is a host Resample[A]
        # (model/package.scala:23): the step is split at the resampler (cssm_pf_propagate / cssm_pf_adopt) and the function
        # is applied to the cloud's columns exactly as the reference applies it to its Vector[State] -- a parity path.
        self._resampler = kinds.get(resample, 0)
        self._host_resample = None if resample in kinds else resample
        self.mod = mod
        self.resample = resample
        self.seed = seed
        self.device = device
        self._pf: Optional[NativePf] = None
        self._host_step = 0
        if n_particles is not None:
            self._ensure(n_particles)

    def _ensure(self, n: int) -> NativePf:
        if self._pf is None or self._pf.n != n:
            if self._pf is not None:
                self._pf.close()
            self._pf = NativePf(self.mod, n, self.seed, self.device, self.lgcp_precision)
            if self._resampler:
                self._pf.set_option(2, self._resampler)   # CSSM_OPT_RESAMPLER
        return self._pf

    def _state(self, t, obs, ll, ess) -> PfState:
        return PfState(t, obs, ll, ess, self._pf, self._pf.generation)

    # ParticleFilter.scala:105-108
    def initialiseState(self, particles: int, t0: float) -> PfState:
        pf = self._ensure(particles)
        pf.init(t0)
        self._host_step = 0                                 # weighted observations resampled on the host since the cloud was drawn
        return self._state(t0, None, 0.0, particles)

    # ParticleFilter.scala:116-132 (FilterLgcp: :210-226)
    def stepFilter(self, s: PfState, y: TimedObservation) -> PfState:
        if s._owner is not self._pf or s._generation != self._pf.generation:
            raise RuntimeError("stepFilter must be applied to the filter's current PfState")
        if self._host_resample is not None:
            return self._step_with_host_resampler(s, y)
        ll, ess = self._pf.step(y.t, y.observation)
        return self._state(y.t, y.observation, ll, ess)

    def _step_with_host_resampler(self, s: PfState, y: TimedObservation) -> PfState:
        """stepFilter with the user's Resample[A], line by line (ParticleFilter.scala:116-132): the device propagates and
        weighs, the host rescales by the max, resamples with the given function and computes ll and ess."""
        pf = self._pf
        weighted = y.observation is not None or self.lgcp_precision > 0
        pf.propagate(y.t, y.observation)
        if not weighted:                                   # :121
            return self._state(y.t, y.observation, s.ll, s.ess)
        w = pf.logw()                                      # :123
        x1 = pf.proposed()
        mx = float(np.max(w))                              # :124
        w1 = np.exp(w - mx)                                # :125
        cols = [x1[:, i] for i in range(pf.n)]
        if self._host_resample is Resampling.residualResampling:
            # the residual extension draws its remainder from counter-based variates: keyed by the FILTER's seed and the observation's
            # index like the three native resamplers, so that Filter(seed = ...) reproduces (unkeyed it took a fresh seed per step)
            new = Resampling.residualResampling(cols, w1, seed=self.seed, step=self._host_step)
        else:
            new = self._host_resample(cols, w1)            # :126
        self._host_step += 1
        if len(new) != pf.n:
            raise ValueError("the resampler must return as many particles as it was given")
        ll = s.ll + mx + math.log(float(np.sum(w1)) / pf.n)   # :127
        nw = w1 / np.sum(w1)
        ess = int(math.floor(1.0 / float(np.sum(nw * nw))))   # :128
        pf.adopt(np.stack(new, axis=1), ll, ess)
        return self._state(y.t, y.observation, ll, ess)

    # ParticleFilter.scala:137-140
    def llFilter(self, data: Sequence[TimedObservation], n: int) -> float:
        if self._host_resample is not None:                # fold stepFilter over the data (:137-140)
            st = self.initialiseState(n, min(d.t for d in data))
            for d in data:
                st = self.stepFilter(st, d)
            return st.ll
        t, y, h = split_data(data)
        return self._ensure(n).run(t, y, h)[0]

    # ParticleFilter.scala:152-158
    def filter(self, data: Sequence[TimedObservation], particles: int) -> Tuple[float, List[StateSpace]]:
        if self._host_resample is not None:                # scan stepFilter, one uniformly picked particle per state (:152-158)
            rng = np.random.default_rng(self.seed)
            t0 = min(d.t for d in data)
            st = self.initialiseState(particles, t0)
            out = [StateSpace(t0, self._pf.particles()[:, int(rng.integers(particles))].copy())]
            for d in data:
                st = self.stepFilter(st, d)
                out.append(StateSpace(d.t, self._pf.particles()[:, int(rng.integers(particles))].copy()))
            return st.ll, out
        t, y, h = split_data(data)
        ll, _, _, path = self._ensure(particles).run(t, y, h, want_path=True)
        times = [float(np.min(t))] + [float(v) for v in t]
        return ll, [StateSpace(tt, path[i].copy()) for i, tt in enumerate(times)]

    # examples/Filtering.scala:23-32: filter, then getIntervals of every emitted state
    def _batch_intervals(self, pf: NativePf, t, y, h, interval: float):
        """(ll, rows) of the batch path: the six row arrays of T + 1 entries (cssm_pf_filter_intervals)."""
        r = pf.filter_intervals(t, y, h, interval)
        return r[0], r[3:]

    def filterIntervals(self, data: Sequence[TimedObservation], particles: int, interval: float = 0.975) -> Tuple[float, List[PfOut]]:
        """``filter`` followed by ``getIntervals`` of every emitted state, in one native call: the log-likelihood and T + 1 ``PfOut`` --
        the first of the initial cloud at the data's smallest time with ``observation = None``, as ``filterStream`` emits the initial
        state, then one per record.  Each equals what ``ParticleFilter.getIntervals`` returns for that state of a ``filterStream`` run
        (at the given ``interval``), so ``formats.pfout_csv`` writes the reference's ``Filtered.csv`` lines from them.
        With a host ``Resample[A]`` (any function but the three native resamplers, the residual extension included) there is no batch
        path: the records go through ``stepFilter`` one by one with a ``summary`` behind each."""
        data = list(data)
        if self._host_resample is not None:
            st = self.initialiseState(particles, min(d.t for d in data))
            outs = [_pfout_of(st.t, None, self._pf.summary(interval))]
            for d in data:
                st = self.stepFilter(st, d)
                outs.append(_pfout_of(d.t, d.observation, self._pf.summary(interval)))
            return st.ll, outs
        t, y, h = split_data(data)
        ll, rows = self._batch_intervals(self._ensure(particles), t, y, h, interval)
        return ll, pfouts_from_rows([float(np.min(t))] + [d.t for d in data], [None] + [d.observation for d in data], rows)

    def stepIntervals(self, s: PfState, y: TimedObservation, interval: float = 0.975) -> Tuple[PfState, PfOut]:
        """``stepFilter`` and ``getIntervals`` of the state it returns, in one native call (cssm_pf_step_intervals; with a host
        ``Resample[A]``: ``stepFilter``, then ``summary``)."""
        if s._owner is not self._pf or s._generation != self._pf.generation:
            raise RuntimeError("stepIntervals must be applied to the filter's current PfState")
        if self._host_resample is not None:
            st = self.stepFilter(s, y)
            return st, _pfout_of(y.t, y.observation, self._pf.summary(interval))
        r = self._pf.step_intervals(y.t, y.observation, interval=interval)
        return self._state(y.t, y.observation, r[0], r[1]), _pfout_of(y.t, y.observation, r[2:])

    # ParticleFilter.scala:389-409 mapped over the filter stream: the forecast of every record's time from the state before it
    def _batch_forecasts(self, pf: NativePf, t, y, h, interval: float):
        """The dict of the batch path (cssm_pf_filter_forecasts): T rows, the first from the initial cloud at the data's smallest time."""
        return pf.filter_forecasts(t, y, h, None, interval)

    def filterForecasts(self, data: Sequence[TimedObservation], particles: int, interval: float = 0.975) -> Tuple[float, List[ForecastOut]]:
        """The prequential check in one native call: the log-likelihood and T ``ForecastOut``, entry s what
        ``ParticleFilter.getMeanForecast(state before record s, mod, data[s].t, interval)`` returns on a ``filterStream`` run, formed before
        record s is weighed, so ``formats.forecast_out_csv`` writes the same lines.  With a host ``Resample[A]`` (any function but the
        three native resamplers) there is no batch path: the loop of ``getMeanForecast`` then ``stepFilter`` runs record by record.
        ``FilterLgcp`` raises the library's refusal (``CssmError``): the reference's ``LogGaussianCox.observation`` is unimplemented."""
        data = list(data)
        if self._host_resample is not None:
            st = self.initialiseState(particles, min(d.t for d in data))
            outs = []
            for d in data:
                outs.append(ParticleFilter.getMeanForecast(st, self.mod, d.t, interval))
                st = self.stepFilter(st, d)
            return st.ll, outs
        t, y, h = split_data(data)
        r = self._batch_forecasts(self._ensure(particles), t, y, h, interval)
        return r["ll"], _forecast_outs([d.t for d in data], r)

    def stepForecast(self, s: PfState, y: TimedObservation, interval: float = 0.975) -> Tuple[PfState, ForecastOut]:
        """``getMeanForecast(s, mod, y.t, interval)`` and ``stepFilter(s, y)`` in one native call (cssm_pf_step_forecast; with a host
        ``Resample[A]``: the two calls)."""
        if s._owner is not self._pf or s._generation != self._pf.generation:
            raise RuntimeError("stepForecast must be applied to the filter's current PfState")
        if self._host_resample is not None:
            out = ParticleFilter.getMeanForecast(s, self.mod, y.t, interval)
            return self.stepFilter(s, y), out
        ll, ess, fc = self._pf.step_forecast(y.t, y.observation, interval=interval)
        return self._state(y.t, y.observation, ll, ess), _forecast_outs([y.t], fc)[0]

    # ParticleFilter.scala:163-166: Flow[Data].scan(init)(stepFilter) -- emits init, then one state per datum
    def filterStream(self, t0: float, particles: int) -> Callable[[Iterable[TimedObservation]], Iterator[PfState]]:
        def flow(source: Iterable[TimedObservation]) -> Iterator[PfState]:
            s = self.initialiseState(particles, t0)
            yield s
            for y in source:
                s = self.stepFilter(s, y)
                yield s
        return flow


class Filter(_FilterBase):
    """``Filter(mod, resample)``, ParticleFilter.scala:233-246."""


class FilterInit(_FilterBase):
    """``FilterInit(mod, resample, initState)``, ParticleFilter.scala:252-271."""

    def __init__(self, mod: Model, resample, initState: Sequence[float], **kw):
        super().__init__(mod, resample, **kw)
        self.initState = np.asarray(initState, dtype=np.float64)

    def initialiseState(self, particles: int, t0: float) -> PfState:
        pf = self._ensure(particles)
        pf.init_from(t0, self.initState)
        return self._state(t0, None, 0.0, particles)

    def llFilter(self, data: Sequence[TimedObservation], n: int) -> float:
        """llFilter (:137-140) folds stepFilter from THIS class's initialiseState: the given state at the data's smallest time, then the
        records in one native call (cssm_pf_ll_filter_more)."""
        if self._host_resample is not None:
            return super().llFilter(data, n)
        t, y, h = split_data(data)
        self.initialiseState(n, float(np.min(t)))
        return self._pf.run_more(t, y, h)[0]

    def _batch_intervals(self, pf: NativePf, t, y, h, interval: float):
        """The given state at the data's smallest time and its summary (row 0), then the records with their rows in one native call
        (cssm_pf_filter_intervals_more)."""
        self.initialiseState(pf.n, float(np.min(t)))
        first = pf.summary(interval)
        r = pf.filter_intervals_more(t, y, h, interval)
        return r[0], tuple(np.concatenate([np.asarray(a)[None], b]) for a, b in zip(first, r[3:]))

    def _batch_forecasts(self, pf: NativePf, t, y, h, interval: float):
        """The given state at the data's smallest time, then the records with their forecasts in one native call
        (cssm_pf_filter_forecasts_more)."""
        self.initialiseState(pf.n, float(np.min(t)))
        return pf.filter_forecasts_more(t, y, h, None, interval)


class FilterLgcp(_FilterBase):
    """``FilterLgcp(mod, resample, precision)``, ParticleFilter.scala:169-227."""

    def __init__(self, mod: Model, resample, precision: int, **kw):
        self.lgcp_precision = int(precision)
        super().__init__(mod, resample, **kw)


class FilterInterpolate(_FilterBase):
    """``FilterInterpolate(mod, resample)``, ParticleFilter.scala:273-311: particles are whole paths and a weighted
    step resamples the paths.  The reference's only consumer (examples/Interpolate.scala:34-44) runs the stream to
    the end and summarises the LAST state's transposed paths; ``interpolate`` returns exactly that list of ``PfOut``
    (one per emitted state: the initial one and one per datum), formed on the device from the ancestor history.

    ``reference_pairing=True`` reproduces the example's ``zipped`` literally: the transposed paths run newest-first,
    so entry k carries the time/observation of index k but the states of index T-k; the default pairs them
    chronologically, which is what the example means to plot."""

    def interpolate(self, data: Sequence[TimedObservation], particles: int, interval: float = 0.975,
                    reference_pairing: bool = False) -> Tuple[float, List[PfOut]]:
        t, y, h = split_data(data)
        ll, *arrays = self._ensure(particles).interpolate(t, y, h, interval, reference_pairing)
        return ll, _interpolate_outs(data, t, arrays)

    def smooth(self, data: Sequence[TimedObservation], particles: int, n_traj: Optional[int] = None,
               interval: float = 0.975) -> Tuple[float, List[PfOut]]:
        """EXTENSION (the reference has none): forward filtering, backward simulation -- ``interpolate``'s forward pass, then ``n_traj``
        trajectories (None: min(particles, 4096)) drawn backwards through the kept clouds (``NativePf.smooth``).  Returns what
        ``interpolate`` returns, in the chronological pairing."""
        t, y, h = split_data(data)
        ll, *arrays = self._ensure(particles).smooth(t, y, h, n_traj, interval)
        return ll, _interpolate_outs(data, t, arrays)

    def window(self, slices: int):
        """``NativePf.window`` on the filter's handle (``initialiseState`` or ``n_particles`` first): the device memory ``stepInterpolate``
        remembers in (0 frees it)."""
        if self._pf is None:
            raise RuntimeError("window needs the filter's handle: initialiseState (or n_particles) first")
        self._pf.window(slices)
        self._win_hist = []

    def stepInterpolate(self, s: PfState, y: TimedObservation, lag: Optional[int], interval: float = 0.975) -> Tuple[PfState, List[PfOut]]:
        """The stream itself (``ParticleFilter.interpolate``, ParticleFilter.scala:281-310), one element per call: ``stepFilter``, and the
        ``PfOut`` of the last ``lag + 1`` time indices through the paths that survive to this datum, oldest first as ``interpolate``
        returns them (fewer while the window holds fewer; ``lag=None``: an empty list).  ``window(slices)`` first; one of the three
        native resamplers."""
        if self._pf is None or s._owner is not self._pf or s._generation != self._pf.generation:
            raise RuntimeError("stepInterpolate must be applied to the filter's current PfState")
        if self._host_resample is not None:
            raise RuntimeError("stepInterpolate remembers the device's ancestors: it needs one of the three native resamplers")
        hist = getattr(self, "_win_hist", [])             # the (t, observation) of the window's slices, oldest first
        if self._pf.window_depth() == 0:                   # a window that restarts takes the state before this datum as its base slice
            hist = [(s.t, s.observation)]
        ll, ess, nrows, rows = self._pf.step_interpolate(y.t, y.observation, lag=lag, interval=interval)
        hist = (hist + [(y.t, y.observation)])[-(self._pf.window_depth() + 1):]
        self._win_hist = hist
        return self._state(y.t, y.observation, ll, ess), [_pfout(*hist[-1 - j], rows, j) for j in range(nrows - 1, -1, -1)]


@dataclass(frozen=True)
class FleetState:
    """``PfState`` of one series of a ``FilterFleet`` (ParticleFilter.scala:32-37); ``particles`` is fetched on demand and only for
    the fleet's current state."""
    t: float
    observation: Optional[float]
    ll: float
    ess: int
    series: int = 0
    _owner: Optional[NativePfFleet] = field(default=None, repr=False, compare=False)
    _generation: int = field(default=-1, repr=False, compare=False)

    @property
    def particles(self) -> np.ndarray:
        if self._owner is None or self._owner.generation != self._generation:
            raise RuntimeError("this state is not the fleet's current one; its cloud was advanced on the device")
        return self._owner.particles(self.series)


class FilterFleet:
    """The reference's streaming filter per sensor (``filterStream``, ParticleFilter.scala:163-166) for many sensors at once:
    ``Filter(mods[k], resample)`` for every k, advanced by one device call.  ``mods`` share one structure; series k's default key is
    ``cssm_pf_run_key(seed, k)``.  Only ``Resampling.systematicResampling`` is served: any other ``resample`` raises with the
    C layer's message (``Filter`` / ``NativePfBatch`` serve the others)."""

    def __init__(self, mods: Sequence[Model], resample, n_particles: int, seed: int = 20260101, device: int = 0):
        if not callable(resample):
            raise TypeError("resample must be a Resample[A]: (samples, weights) -> samples")
        kinds = {Resampling.systematicResampling: 0, Resampling.stratifiedResampling: 1, Resampling.multinomialResampling: 2}
        self.mods = list(mods)
        self.S = len(self.mods)
        self.seed = seed
        self._fleet = self._new_fleet(self.mods[0], n_particles, self.S, device)
        try:
            self._fleet.set_option(2, kinds.get(resample, 3))      # CSSM_OPT_RESAMPLER: refused unless systematic
            self._fleet.set_params(self.mods)
            self._fleet.reseed(self.keys(seed, self.S))
        except Exception:
            self._fleet.close()
            raise
        self._states: List[FleetState] = []

    def _new_fleet(self, mod: Model, n: int, series: int, device: int) -> NativePfFleet:
        return NativePfFleet(mod, n, series, device)

    @staticmethod
    def keys(seed: int, series: int) -> List[int]:
        """Series k runs under ``cssm_pf_run_key(seed, k)`` -- never ``seed + k`` (include/cssm_pf.h, cssm_pf_run_key)."""
        lib = _abi.load_library()
        return [int(lib.cssm_pf_run_key(int(seed) & (2**64 - 1), k)) for k in range(int(series))]

    def close(self):
        self._fleet.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _wrap(self, t, obs, ll, ess) -> List[FleetState]:
        g = self._fleet.generation
        self._states = [FleetState(float(t[k]), obs[k], float(ll[k]), int(ess[k]), k, self._fleet, g) for k in range(self.S)]
        return self._states

    def initialiseState(self, t0s) -> List[FleetState]:
        t0 = np.broadcast_to(np.asarray(t0s, dtype=np.float64), (self.S,))
        self._fleet.init(t0)
        return self._wrap(t0, [None] * self.S, np.zeros(self.S), [self._fleet.n] * self.S)

    def initialiseStateFrom(self, t0s, states, seed: Optional[int] = None) -> List[FleetState]:
        """``FilterInit(mods[k], resample, states[k]).initialiseState`` of every series, or its posterior form, in one device call: each
        entry of ``states`` is one state ``[d]`` (replicated) or the ``last_state`` array ``[M_k, d]`` of a posterior -- the second element
        of each pair from ``pmmh.fleet_posterior_rows`` is accepted as it is --, its states at ``t0s[k]``; particle i then starts at the
        row ``forecastPosterior`` selects for it.  seed = the Philox key of every series' selection; None: each series' default key
        (``NativePfFleet.posterior_key``)."""
        t0 = np.broadcast_to(np.asarray(t0s, dtype=np.float64), (self.S,))
        keys = [self._fleet.posterior_key(k) for k in range(self.S)] if seed is None else [int(seed)] * self.S
        _, rc = self._fleet.init_from(t0, states, keys=keys)
        for k in range(self.S):
            if rc[k]:
                raise _abi.CssmError(int(rc[k]), self._fleet.lib.cssm_last_error().decode() or f"series {k}: its states were refused")
        return self._wrap(t0, [None] * self.S, np.zeros(self.S), [self._fleet.n] * self.S)

    def _more(self, datas, call):
        """What both continuing calls do around theirs: one (possibly empty) list of data per series, the series' own statuses raised,
        the states of before forgotten.  Returns ``(split data, what the call returned)``."""
        split = [split_data(d) if len(d) else (np.zeros(0), np.zeros(0), None) for d in datas]
        out = call(split)
        self._raise_series(out[-1], stepping=True)
        self._states = []
        return split, out

    def llFilterMore(self, datas: Sequence[Sequence[TimedObservation]]) -> np.ndarray:
        """The next data of every running series in one device call (one launch; ``datas[k]`` may be empty): the log-likelihoods
        accumulated since the series were initialised (NaN for a series without new data)."""
        return self._more(datas, self._fleet.ll_filter_more)[1][0]

    def filterIntervalsMore(self, datas: Sequence[Sequence[TimedObservation]], interval: float = 0.975) -> List[List[PfOut]]:
        """``llFilterMore`` mapped through ``getIntervals``, from the same launch: per series one ``PfOut`` per datum, as
        ``filterIntervals`` returns them behind its first."""
        split, out = self._more(datas, lambda sp: self._fleet.filter_intervals_more(sp, float(interval)))
        return [[_pfout(d.t, d.observation, out[3][k], i) for i, d in enumerate(datas[k])] for k in range(self.S)]

    def stepFilter(self, states: Sequence[FleetState], ys: Sequence[Optional[TimedObservation]]) -> List[FleetState]:
        """``ys[k]`` None = sensor k has nothing new (its state is returned as it is); a TimedObservation whose ``observation`` is None
        is the reference's ``None`` branch (propagate only)."""
        return self._advance(states, ys, lambda t, y, has, act: self._fleet.step(t, y, has, act) + (None,))[0]

    def stepIntervals(self, states: Sequence[FleetState], ys: Sequence[Optional[TimedObservation]],
                      interval: float = 0.975) -> Tuple[List[FleetState], List[Optional[PfOut]]]:
        """``stepFilter`` and ``getIntervals`` of every state it advanced, from one device call (``filterStream`` mapped through
        ``getIntervals``, examples/Filtering.scala:24-31): the new states, and per series its ``PfOut`` -- None where ``ys[k]`` is None."""
        def call(t, y, has, act):
            ll, ess, rows, rc = self._fleet.step_intervals(t, y, has, act, float(interval))
            return ll, ess, rc, rows
        new, act, rows = self._advance(states, ys, call)
        return new, [_pfout(new[k].t, new[k].observation, rows, k) if act[k] else None for k in range(self.S)]

    def stepForecast(self, states: Sequence[FleetState], ys: Sequence[Optional[TimedObservation]],
                     interval: float = 0.975) -> Tuple[List[FleetState], List[Optional[ForecastOut]]]:
        """``getMeanForecast`` of every datum's time from the state before it, then ``stepFilter``, from one device call
        (``ParticleFilter.getMeanForecast`` mapped over a ``filterStream``, :368-409): the new states, and per series the
        ``ForecastOut`` at its datum's time under the series' default key -- None where ``ys[k]`` is None."""
        def call(t, y, has, act):
            ll, ess, fc, rc, fc_rc = self._fleet.step_forecast(t, y, has, act, None, float(interval))
            self._raise_series(None, fc_rc=fc_rc, stepping=True)
            return ll, ess, rc, fc
        new, act, fc = self._advance(states, ys, call)
        return new, [_forecast_outs([new[k].t], {name: v[k:k + 1] for name, v in fc.items()})[0] if act[k] else None for k in range(self.S)]

    def window(self, slices: int):
        """``NativePfFleet.window``: the device memory ``stepInterpolate`` remembers in (0 frees it)."""
        self._fleet.window(slices)
        self._win_hist = [[] for _ in range(self.S)]

    def stepInterpolate(self, states: Sequence[FleetState], ys: Sequence[Optional[TimedObservation]], lag,
                        interval: float = 0.975) -> Tuple[List[FleetState], List[List[PfOut]]]:
        """``FilterInterpolate``'s stream (``ParticleFilter.interpolate``, ParticleFilter.scala:281-310) per sensor: ``stepFilter``, and per
        series the ``PfOut`` of its last ``lag + 1`` time indices through the paths that survive to this datum, oldest first as
        ``interpolate`` returns them (fewer while the window holds fewer; an empty list where ``ys[k]`` is None).  ``lag``: an int, or
        one entry per series with None for "no rows".  ``window(slices)`` first."""
        if np.ndim(lag) == 0:
            lag = [lag] * self.S
        if len(lag) != self.S:
            raise ValueError(f"one lag per series ({self.S}), not {len(lag)}")
        max_lag = max([int(v) for v in lag if v is not None], default=0)
        hist = getattr(self, "_win_hist", None) or [[] for _ in range(self.S)]   # per series the (t, observation) of its window's slices

        def call(t, y, has, act):
            for k in range(self.S):                    # a window that restarts takes the state before this datum as its base slice
                if act[k] and self._fleet.window_depth(k) == 0:
                    hist[k] = [(states[k].t, states[k].observation)]
            ll, ess, nrows, rows, rc = self._fleet.step_interpolate(t, y, has, act, list(lag), max_lag, float(interval))
            return ll, ess, rc, (nrows, rows)
        new, act, (nrows, rows) = self._advance(states, ys, call)
        outs = []
        for k in range(self.S):
            if not act[k]:
                outs.append([]); continue
            hist[k] = (hist[k] + [(new[k].t, new[k].observation)])[-(self._fleet.window_depth(k) + 1):]
            outs.append([_pfout(*hist[k][-1 - j], rows, (k, j)) for j in range(int(nrows[k]) - 1, -1, -1)])
        self._win_hist = hist
        return new, outs

    def _advance(self, states, ys, call):
        """What every step method does around its device call: the fleet's current states and one (optional) observation per series or
        a refusal; ``call(t, y, has, act)`` -> ``(ll, ess, rc, rest)``; a series' own status raised; the new states (an inactive
        series keeps the fields of its old one).  Returns ``(new_states, act, rest)``."""
        if len(states) != self.S or len(ys) != self.S:
            raise ValueError("one state and one (optional) observation per series")
        if any(s._owner is not self._fleet or s._generation != self._fleet.generation for s in states):
            raise RuntimeError("stepFilter needs the fleet's current states (the clouds live on the device)")
        act = np.array([0 if o is None else 1 for o in ys], dtype=np.uint8)
        t = np.array([states[k].t if o is None else o.t for k, o in enumerate(ys)], dtype=np.float64)
        has = np.array([0 if (o is None or o.observation is None) else 1 for o in ys], dtype=np.uint8)
        y = np.array([o.observation if h else 0.0 for o, h in zip(ys, has)], dtype=np.float64)
        ll, ess, rc, rest = call(t, y, has, act)
        self._raise_series(rc, stepping=True)
        keep = [s if not a else None for s, a in zip(states, act)]
        new = self._wrap(t, [s.observation if s is not None else (float(y[k]) if has[k] else None) for k, s in enumerate(keep)],
                         [s.ll if s is not None else ll[k] for k, s in enumerate(keep)],
                         [s.ess if s is not None else ess[k] for k, s in enumerate(keep)])
        return new, act, rest

    def _raise_series(self, rc, empty_ok=False, fc_rc=None, stepping=False):
        """Raise the first series' own status, as the reference throws from its filter: ``rc[k]`` -- "it has no records" for
        CSSM_EINVAL_ARG where the call runs a fleet with an empty series (``empty_ok``), else "its weights were unusable" (a step may
        also have met a series without a cloud) --, then ``fc_rc[k]``, a refused forecast, with the library's own text."""
        for k in range(self.S):
            if rc is not None and rc[k]:
                why = ("it has no records" if empty_ok and rc[k] == _abi.CSSM_EINVAL_ARG else
                       "its weights were unusable" + (" (or it has no cloud)" if stepping else ""))
                raise _abi.CssmError(int(rc[k]), f"series {k}: {why}")
            if fc_rc is not None and fc_rc[k]:
                raise _abi.CssmError(int(fc_rc[k]), self._fleet.lib.cssm_last_error().decode()
                                     or f"series {k}: its forecast{' was' if stepping else 's were'} refused")

    def llFilter(self, datas: Sequence[Sequence[TimedObservation]]) -> np.ndarray:
        ll, _, _, rc = self._fleet.ll_filter([split_data(d) for d in datas])
        self._raise_series(rc)
        self._states = []
        return ll

    def filter(self, datas: Sequence[Sequence[TimedObservation]]) -> List[Tuple[float, List[StateSpace]]]:
        """``Filter.filter`` (ParticleFilter.scala:152-158) of every series in one device call: per series ``(ll, [StateSpace(t, state)])``
        of length T_k + 1, the first entry at the slice's smallest time."""
        split = [split_data(d) for d in datas]
        ll, _, _, paths, _, rc = self._fleet.filter(split)
        self._raise_series(rc)
        self._states = []
        out = []
        for k, (t, _, _) in enumerate(split):
            times = [float(np.min(t))] + [float(v) for v in t]
            out.append((float(ll[k]), [StateSpace(tt, paths[k][i].copy()) for i, tt in enumerate(times)]))
        return out

    def filterIntervals(self, datas: Sequence[Sequence[TimedObservation]], interval: float = 0.975) -> List[List[PfOut]]:
        """examples/Filtering.scala:24-31 of every series in one device call (one launch): ``filter`` mapped through ``getIntervals`` --
        per series T_k + 1 ``PfOut``, the first without an observation at the slice's smallest time (``Flow.scan`` emits the initial
        state), entry s + 1 after datum s.  ``formats.pfout_csv`` writes the reference's ``Filtered.csv`` lines from them."""
        split = [split_data(d) for d in datas]
        _, _, _, rows, rc = self._fleet.filter_intervals(split, float(interval))
        self._raise_series(rc, empty_ok=True)
        self._states = []
        return [_interpolate_outs(datas[k], split[k][0], rows[k]) for k in range(self.S)]

    def filterForecasts(self, datas: Sequence[Sequence[TimedObservation]], interval: float = 0.975) -> List[List[ForecastOut]]:
        """``ParticleFilter.getMeanForecast`` (:368-409) mapped over the filter stream of every series in one device call (one launch):
        per series one ``ForecastOut`` per datum, at the datum's time, from the state before the datum and under the key
        ``getMeanForecast`` takes there by default.  ``formats.forecast_out_csv`` writes the reference's lines from them."""
        split = [split_data(d) for d in datas]
        _, _, _, fc, rc, fc_rc = self._fleet.filter_forecasts(split, float(interval))
        self._raise_series(rc, empty_ok=True, fc_rc=fc_rc)
        self._states = []
        return [_forecast_outs([float(v) for v in split[k][0]], fc[k]) for k in range(self.S)]

    def interpolate(self, datas: Sequence[Sequence[TimedObservation]], interval: float = 0.975,
                    reference_pairing: bool = False) -> List[Tuple[float, List[PfOut]]]:
        """``FilterInterpolate(mods[k], resample).interpolate(datas[k], n)`` of every series in one device call (two launches): per series
        ``(ll, [PfOut])`` of length T_k + 1.  The fleet's current states stay valid: the clouds are not touched."""
        split = [split_data(d) for d in datas]
        ll, rows, rc = self._fleet.interpolate(split, float(interval), reference_pairing)
        self._raise_series(rc, empty_ok=True)
        return [(float(ll[k]), _interpolate_outs(datas[k], split[k][0], rows[k])) for k in range(self.S)]

    def interpolate_last_ms(self) -> Tuple[float, float]:
        return self._fleet.interpolate_last_ms()

    def smooth(self, datas: Sequence[Sequence[TimedObservation]], n_traj: Optional[int] = None,
               interval: float = 0.975) -> List[Tuple[float, List[PfOut]]]:
        """An EXTENSION (the reference has no smoother beyond ``FilterInterpolate``): what ``interpolate`` returns, per series ``(ll,
        [PfOut])`` of length T_k + 1, but every time index summarised over ``n_traj`` backward-simulated trajectories (None: as many as
        particles) instead of the lineages that survive to the end of the series -- the early rows of a long series keep a
        distribution.  One device call (three launches); the fleet's current states stay valid."""
        split = [split_data(d) for d in datas]
        ll, rows, rc = self._fleet.smooth(split, n_traj, float(interval))
        self._raise_series(rc, empty_ok=True)
        return [(float(ll[k]), _interpolate_outs(datas[k], split[k][0], rows[k])) for k in range(self.S)]

    def smooth_last_ms(self) -> Tuple[float, float, float]:
        return self._fleet.smooth_last_ms()

    def forecast(self, times, interval: float = 0.975, seed: Optional[int] = None) -> List[List[ForecastOut]]:
        """``ParticleFilter.forecast`` of every series from its current state, all of them in one device call: ``times[k]`` = series k's
        future times (None / empty: none; the list for it is empty).  seed = the Philox key of every series' draws; None: each
        series' default key (``NativePfFleet.forecast_key``)."""
        ts = [[] if v is None else [float(x) for x in v] for v in times]
        rs = self._fleet.forecast(ts, None if seed is None else [int(seed)] * self.S, float(interval))
        for k, r in enumerate(rs):
            if r["rc"]:
                raise _abi.CssmError(r["rc"], f"series {k}: its forecast was refused (no cloud, times before its clock or decreasing, "
                                              f"or a model without the scale its observation needs)")
        return [_forecast_outs(ts[k], rs[k]) for k in range(self.S)]

    def forecastPosterior(self, posteriors, t0s, times, interval: float = 0.975, seed: Optional[int] = None,
                          params: Optional[Parameters] = None) -> List[List[ForecastOut]]:
        """``ParticleFilter.forecastPosterior`` of every series under its own joint posterior sample -- e.g. the chains of
        ``pmmh.pmmh_native_fleet`` through ``pmmh.fleet_posterior_rows`` --, all of them in one device call: ``posteriors[k]`` is what
        ``ParticleFilter.forecastPosterior`` accepts (MetropStates, or the arrays (theta[M, n_theta], last_state[M, d]) with ``params``,
        the parameter tree the rows flatten), its states at ``t0s[k]``; n = the fleet's particles.  seed = the Philox key of every
        series' draws; None: each series' default key (``NativePfFleet.posterior_key``).  No series needs a filtered state."""
        if len(posteriors) != self.S or len(times) != self.S:
            raise ValueError("one posterior and one array of times per series")
        t0 = np.asarray(t0s, dtype=np.float64)
        if t0.ndim != 0 and t0.shape != (self.S,):
            raise ValueError("one t0 per series (or one for all)")
        ts = [[] if v is None else [float(x) for x in v] for v in times]
        post = [_posterior_arrays(p, params)[:2] for p in posteriors]
        rs = self._fleet.forecast_posterior(post, t0, ts, None if seed is None else [int(seed)] * self.S, float(interval))
        for k, r in enumerate(rs):
            if r["rc"]:
                raise _abi.CssmError(r["rc"], self._fleet.lib.cssm_last_error().decode() or f"series {k}: its posterior forecast was refused")
        return [_forecast_outs(ts[k], rs[k]) for k in range(self.S)]

    def simulate(self, t0s, timess, seed: Optional[int] = None):
        """``SimulateData(mods[k]).simPompModel(t0s[k])(timess[k])`` of every sensor in one device call: per sensor the list of its
        ``simulate.SimulatedPoint`` (the point at t0, then one per time) -- data that ``llFilter`` / ``filter`` take as they are.  Series
        k draws under cssm_pf_run_key(seed_k, 2^62 | k), seed_k its filter key (``seed`` given: that of ``keys(seed, S)``).  The fleet's
        clouds are not touched."""
        from .simulate import fleet_keys, points_of
        seeds = self._fleet.seeds if seed is None else self.keys(seed, self.S)
        t0 = np.broadcast_to(np.asarray(t0s, dtype=np.float64), (self.S,))
        rows, rc = self._fleet.simulate(t0, timess, 1, fleet_keys(seeds))
        self._raise_series(None, fc_rc=rc)
        return [points_of(float(t0[k]), [] if timess[k] is None else timess[k], rows[k]) for k in range(self.S)]

    def getMeanForecast(self, ts, interval: float, seed: Optional[int] = None) -> List[ForecastOut]:
        """``ParticleFilter.getMeanForecast`` (:389-409) of every series: one horizon each, ``ts[k]`` its time."""
        return [o[0] for o in self.forecast([[float(v)] for v in ts], interval, seed)]

    def getIntervals(self) -> List[PfOut]:
        """``ParticleFilter.getIntervals`` (:415-424) of every series' current state."""
        rows = self._fleet.summary(0.975)
        st = self._states if self._states and self._states[0]._generation == self._fleet.generation else None
        return [_pfout(st[k].t if st else float("nan"), st[k].observation if st else None, rows, k, bound=lambda v: v) for k in range(self.S)]


class FilterInitFleet(FilterFleet):
    """``FilterInit(mods[k], resample, initStates[k])`` (ParticleFilter.scala:252-271) for many sensors at once: a ``FilterFleet`` whose
    clouds start as the given states replicated.  ``llFilter`` is two launches: ``init_from`` at each slice's smallest time, then
    ``ll_filter_more``."""

    def __init__(self, mods: Sequence[Model], resample, initStates, n_particles: int, seed: int = 20260101, device: int = 0):
        super().__init__(mods, resample, n_particles, seed, device)
        self.initStates = [np.asarray(s, dtype=np.float64).reshape(1, -1) for s in initStates]
        if len(self.initStates) != self.S:
            self.close()
            raise ValueError("one initial state per series")

    def initialiseState(self, t0s) -> List[FleetState]:
        return self.initialiseStateFrom(t0s, self.initStates)

    def llFilter(self, datas: Sequence[Sequence[TimedObservation]]) -> np.ndarray:
        if any(len(d) == 0 for d in datas):
            raise ValueError("a series has no records (the reference's minBy throws on an empty Vector)")
        self.initialiseState([min(o.t for o in d) for d in datas])
        return self.llFilterMore(datas)


class FilterLgcpFleet(FilterFleet):
    """``FilterLgcp(mods[k], resample, precision)`` (ParticleFilter.scala:169-227) for many event streams at once, advanced by one device
    call: ``FilterFleet`` over a ``NativeLgcpFleet``.  ``initialiseState``, ``stepFilter``, ``llFilter``, ``filter`` and ``getIntervals``
    are served -- every datum is an event, whatever its ``observation`` --; the other methods raise with the library's refusal.  Series
    k's key is ``cssm_pf_run_key(seed, k)``."""

    def __init__(self, mods: Sequence[Model], resample, precision: int, n_particles: int, seed: int = 20260101, device: int = 0):
        self.precision = int(precision)
        super().__init__(mods, resample, n_particles, seed, device)

    def _new_fleet(self, mod: Model, n: int, series: int, device: int) -> NativePfFleet:
        return NativeLgcpFleet(mod, n, series, self.precision, device)


class ParticleFilter:
    """``object ParticleFilter``: Reader-wrapped entry points, ParticleFilter.scala:321-361."""

    @staticmethod
    def filter(resample, t0: float, n: int, **kw):
        return lambda mod: Filter(mod, resample, **kw).filterStream(t0, n)

    @staticmethod
    def filterInit(resample, t0: float, n: int, initState, **kw):
        return lambda mod: FilterInit(mod, resample, initState, **kw).filterStream(t0, n)

    @staticmethod
    def interpolate(resample, t0: float, particles: int, **kw):   # :335-337 (t0 is re-derived from the data as minSink does)
        return lambda mod: (lambda data: FilterInterpolate(mod, resample, **kw).interpolate(list(data), particles))

    @staticmethod
    def filterLlState(data, resample, n: int, **kw):
        return lambda mod: Filter(mod, resample, **kw).filter(data, n)

    @staticmethod
    def likelihood(data, resample, n: int, **kw):
        return lambda mod: Filter(mod, resample, **kw).llFilter(data, n)

    @staticmethod
    def getIntervals(model: Model, s: "PfState") -> PfOut:
        """ParticleFilter.getIntervals (:415-424), evaluated on the device for the handle's current state."""
        m, lo, hi, em, el, eu = ParticleFilter._current(s).summary(0.975)
        return PfOut(s.t, s.observation, em, CredibleInterval(el, eu), m, [CredibleInterval(a, b) for a, b in zip(lo, hi)])

    @staticmethod
    def _current(s: "PfState") -> NativePf:
        if s._owner is None or s._owner.generation != s._generation:
            raise RuntimeError("the cloud summaries need the filter's current PfState (the cloud lives on the device)")
        return s._owner

    # ---- forecasts (ParticleFilter.scala:368-409, Data.scala:196-231): the handle's parameters, one device call
    @staticmethod
    def _forecast_handle(s: "PfState", mod: Model) -> NativePf:
        pf = ParticleFilter._current(s)
        if mod is not pf.model and _model_signature(mod) != _model_signature(pf.model):
            raise ValueError("forecasts use the filter's own model and parameters: `mod` must be the model the filter was built with")
        return pf

    @staticmethod
    def _key(pf: NativePf, seed: Optional[int]) -> int:
        return pf.forecast_key() if seed is None else int(seed)

    @staticmethod
    def getForecast(s: "PfState", mod: Model, t: float, seed: Optional[int] = None) -> ObservationWithState:
        """getForecast (:368-387): every particle pushed to t, gamma = f(x, t), eta = link(gamma), one observation draw -- as arrays."""
        pf = ParticleFilter._forecast_handle(s, mod)
        r = pf.forecast([t], ParticleFilter._key(pf, seed), 0.975, want_samples=True)
        sm = r["samples"][0]
        d = pf.d
        return ObservationWithState(float(t), sm[d + 2].copy(), sm[d + 1].copy(), sm[d].copy(), sm[:d].copy())

    @staticmethod
    def getMeanForecast(s: "PfState", mod: Model, t: float, interval: float, seed: Optional[int] = None) -> ForecastOut:
        """getMeanForecast (:389-409), the observations drawn once."""
        return ParticleFilter.forecast(s, mod, [t], interval, seed)[0]

    @staticmethod
    def forecast(s: "PfState", mod: Model, times: Sequence[float], interval: float = 0.975, seed: Optional[int] = None) -> List[ForecastOut]:
        """SimulateData.forecast + summariseForecast (Data.scala:196-231): horizon h starts from horizon h - 1's states; one ForecastOut
        per time, all formed in one device call."""
        pf = ParticleFilter._forecast_handle(s, mod)
        times = [float(v) for v in times]
        r = pf.forecast(times, ParticleFilter._key(pf, seed), float(interval))
        return _forecast_outs(times, r)

    @staticmethod
    def forecastPosterior(posterior, unparam: UnparamModel, t0: float, times: Sequence[float], n: int, interval: float = 0.975,
                          seed: Optional[int] = None, params: Optional[Parameters] = None) -> List[ForecastOut]:
        """SimulateData.forecast(unparamModel, t, n)(posterior) + summariseForecast (Data.scala:196-231): n particles, each on a pair
        (theta, x) drawn from the joint posterior sample, pushed from t0 through `times` under its own parameters; one ForecastOut per
        time, all formed in one device call.  `posterior`: MetropStates (e.g. formats.read_pmmh_json(path, burn_in, thin)), or the
        arrays (theta[M, n_theta], last_state[M, d]) of pmmh_native* (pmmh.posterior_rows selects burn-in and thinning) with `params`
        the parameter tree the rows flatten.  seed = the Philox key of the draws; None: the default key of a fresh filter."""
        theta, x, template = _posterior_arrays(posterior, params)
        pf = NativePf(unparam.run(template.withFlat(theta[0])), int(n))
        try:
            times = [float(v) for v in times]
            r = pf.forecast_posterior(theta, x, float(t0), times, pf.forecast_key() if seed is None else int(seed), float(interval))
        finally:
            pf.close()
        return _forecast_outs(times, r)

    @staticmethod
    def meanState(s: "PfState") -> np.ndarray:
        """ParticleFilter.meanState (:475-477) of the state's cloud: per-component means, formed on the device."""
        return ParticleFilter._current(s).summary(0.975)[0]

    @staticmethod
    def getallCredibleIntervals(s: "PfState", interval: float) -> List[CredibleInterval]:
        """ParticleFilter.getallCredibleIntervals (:510-512, getCredibleInterval :488-502) of the state's cloud: per component
        the order statistics sorted(n - index - 1) and sorted(index - 1), index = floor(interval n), selected on the device."""
        _, lo, hi, _, _, _ = ParticleFilter._current(s).summary(float(interval))
        return [CredibleInterval(a, b) for a, b in zip(lo, hi)]

    @staticmethod
    def getOrderStatistic(samples: Sequence[float], interval: float) -> CredibleInterval:
        """ParticleFilter.getOrderStatistic (:455-460) for a vector the caller already holds on the host:
        CredibleInterval(sorted(n - index), sorted(index)), index = floor(n interval).  (The eta intervals of a cloud come
        from getIntervals, which selects them on the device.)"""
        a = np.sort(np.asarray(samples, dtype=np.float64))
        index = int(np.floor(a.size * interval))
        return CredibleInterval(float(a[a.size - index]), float(a[index]))

    @staticmethod
    def effectiveSampleSize(weights: Sequence[float]) -> int:  # :431-434 (host helper, tiny inputs)
        w = np.asarray(weights, dtype=np.float64)
        nw = w / w.sum()
        return int(np.floor(1.0 / np.sum(nw * nw)))

    @staticmethod
    def mean(s: Sequence[float]) -> float:  # :522-524
        return float(np.sum(s)) / len(s)


def _interpolate_outs(data: Sequence[TimedObservation], t, arrays) -> List[PfOut]:
    """The ``PfOut`` list of one interpolated series (examples/Interpolate.scala:42-44) from ``(mean[T + 1, d], lower, upper,
    eta_of_mean[T + 1], eta_lower, eta_upper)``: entry 0 at the smallest time without an observation, entry s + 1 datum s."""
    times = [float(np.min(t))] + [float(v) for v in t]
    obs = [None] + [d.observation for d in data]
    return [_pfout(times[k], obs[k], arrays, k) for k in range(len(times))]


def _pfout(t, obs, arrays, index, bound=float) -> PfOut:
    """The ``PfOut`` at ``(t, obs)`` of row ``index`` of ``(mean, lower, upper, eta_of_mean, eta_lower, eta_upper)``, the state a copy
    (``bound``: what a state interval's bounds are made of -- ``getIntervals`` hands numpy's scalars on as they are)."""
    m, lo, hi, em, el, eu = arrays
    return PfOut(t, obs, float(em[index]), CredibleInterval(float(el[index]), float(eu[index])), m[index].copy(),
                 [CredibleInterval(bound(a), bound(b)) for a, b in zip(lo[index], hi[index])])


def _forecast_outs(times: Sequence[float], r) -> List[ForecastOut]:
    """One ForecastOut per time from the per-horizon arrays of NativePf.forecast / forecast_posterior."""
    return [ForecastOut(tt, float(r["obs_mean"][h]), CredibleInterval(float(r["obs_lower"][h]), float(r["obs_upper"][h])),
                        float(r["eta_mean"][h]), CredibleInterval(float(r["eta_lower"][h]), float(r["eta_upper"][h])),
                        r["state_mean"][h].copy(),
                        [CredibleInterval(float(a), float(b)) for a, b in zip(r["state_lower"][h], r["state_upper"][h])])
            for h, tt in enumerate(times)]


def _posterior_arrays(posterior, params: Optional[Parameters]):
    """(theta[M, n_theta], x[M, d], a parameter tree of the rows' shape) from MetropStates or from (theta, last_state) arrays."""
    if isinstance(posterior, tuple) and len(posterior) == 2 and not hasattr(posterior[0], "params"):
        if params is None:
            raise ValueError("a posterior given as (theta, last_state) arrays needs `params`, the parameter tree its rows flatten")
        theta = np.atleast_2d(np.asarray(posterior[0], dtype=np.float64))
        x = np.asarray(posterior[1], dtype=np.float64).reshape(theta.shape[0], -1)
        template = params
    else:
        states = list(posterior)
        if not states:
            raise ValueError("the posterior sample is empty")
        if any(s.sde is None for s in states):
            raise ValueError("every MetropState needs its sampled state (sde)")
        theta = np.array([s.params.flattenParams() for s in states], dtype=np.float64)
        x = np.array([np.asarray(s.sde, dtype=np.float64).ravel() for s in states])
        template = states[0].params
    if theta.shape[0] == 0:
        raise ValueError("the posterior sample is empty")
    return np.ascontiguousarray(theta), np.ascontiguousarray(x), template


def _model_signature(mod: Optional[Model]):
    """Structure and stored parameters of a model as its descriptor states them (two models that drive a handle identically)."""
    if mod is None:
        return None
    desc = mod.descriptor()
    arr = lambda p, k: tuple(p[i] for i in range(k)) if k else ()
    leaves = tuple((L.sde_kind, L.dim, L.f_kind, L.period, L.harmonics, L.has_scale, L.scale, arr(L.m0, L.n_m0), arr(L.c0, L.n_c0),
                    arr(L.mu, L.n_mu), arr(L.phi, L.n_phi), arr(L.sigma, L.n_sigma)) for L in desc.leaf_array)
    return (desc.desc.obs_kind, desc.desc.obs_df, leaves)
