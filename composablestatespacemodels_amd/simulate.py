"""Series drawn from the model itself, on the device: the reference's ``SimulateData`` (model/Data.scala:53-100, ``simStep`` :186-193;
examples/Simulation.scala) over ``cssm_simulate`` / ``cssm_simulate_from`` (include/cssm_pf.h; csrc/cssm_simulate.hip).

Low level: ``simulate`` (n_paths realisations over given times, rows ``[T + 1, d + 3, n_paths]``: the d states, gamma, eta, obs) and
``simulate_from`` (the same paths continued from given states under consecutive step indices).  The reference's surface:
``SimulateData(model).simPompModel(t0)(times)``, ``.simMarkov(dt)`` / ``.simRegular(dt)`` / ``.observations`` (lazy, simulated in blocks
of rows on the device) and ``.simStep(dt)``, all returning ``SimulatedPoint`` -- one ``ObservationWithState`` (Data.scala:31-36).

Event series of a log-Gaussian Cox process come from ``cssm_simulate_lgcp`` (csrc/cssm_simulate_lgcp.hip), the reference's thinning
(``simLGCP``, Data.scala:110-149): ``simulate_lgcp`` (n_paths realisations, an ``LgcpSim``), ``SimulateData(model).simLGCP(start, end,
precision)`` (one path, the reference's vector) and ``lgcp_events_data`` (the chronological events as a filter takes them).

Keys.  ``SimulateData(model, seed)`` draws under ``cssm_pf_run_key(seed, 2^62)``; a fleet's series k under
``cssm_pf_run_key(seed_k, 2^62 | k)`` (``fleet_keys``).  Run numbers with bit 62 set and bit 63 clear are taken by nothing else: filters
run under ``cssm_pf_run_key(seed, k)`` with k a small series or chain index, forecasts under ``cssm_pf_run_key(seed, 2^63 | observation
index)``.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Callable, Iterable, Iterator, List, Optional, Sequence, Union

import numpy as np

from . import _abi
from ._abi import CssmError
from .model import Model, TimedObservation

SIM_RUN = 1 << 62
_U64 = 2**64 - 1
_dp = C.POINTER(C.c_double)


@dataclass(frozen=True)
class SimulatedPoint:  # ObservationWithState, Data.scala:31-36 (filter.ObservationWithState is struct-of-arrays over a cloud; this is one point)
    t: float
    observation: Optional[float]
    eta: float
    gamma: float
    sdeState: np.ndarray

    def to_data(self) -> TimedObservation:
        return TimedObservation(self.t, self.observation)


def sim_key(seed: int, k: int = 0) -> int:
    """The Philox key of a simulation under user seed ``seed``: cssm_pf_run_key(seed, 2^62 | k)."""
    return int(_abi.load_library().cssm_pf_run_key(int(seed) & _U64, SIM_RUN | int(k)))


def fleet_keys(seeds: Sequence[int]) -> List[int]:
    """Series k's default key from its seed: cssm_pf_run_key(seeds[k], 2^62 | k)."""
    return [sim_key(s, k) for k, s in enumerate(seeds)]


def _times(times) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(list(times) if not isinstance(times, np.ndarray) else times, dtype=np.float64).ravel())


def simulate(model: Model, t0: float, times, n_paths: int = 1, key: Optional[int] = None, device: int = 0, rows_per_launch: int = 0) -> np.ndarray:
    """cssm_simulate: ``[T + 1, d + 3, n_paths]`` -- time index 0 is ``t0``, index h >= 1 is ``times[h - 1]``; per time index the d states,
    gamma, eta and the observation of every path.  ``key``: the Philox key (None: ``sim_key(20260101)``)."""
    lib = _abi.load_library()
    desc = model.descriptor()
    t = _times(times)
    d = sum(int(L.dim) for L in desc.leaf_array)
    out = np.zeros((len(t) + 1, d + 3, int(n_paths)))
    key = sim_key(20260101) if key is None else int(key) & _U64
    tt = t if len(t) else np.zeros(1)
    _abi.check(lib.cssm_simulate(desc.ptr(), int(n_paths), key, float(t0), tt.ctypes.data_as(_dp), len(t), int(rows_per_launch), int(device),
                                 out.ctypes.data_as(_dp)))
    return out


def simulate_from(model: Model, x, first_step: int, t0: float, times, key: int, device: int = 0, rows_per_launch: int = 0) -> np.ndarray:
    """cssm_simulate_from: the paths stand at ``x`` (``[d, n_paths]``, or ``[d]`` for one path) at ``t0`` and move through ``times``; time
    index j of the call moves and draws under step ``first_step + j``.  ``[T, d + 3, n_paths]`` (no row at t0)."""
    lib = _abi.load_library()
    desc = model.descriptor()
    t = _times(times)
    xx = np.asarray(x, dtype=np.float64)
    xx = np.ascontiguousarray(xx.reshape(xx.shape[0], -1))
    d, n = xx.shape
    out = np.zeros((len(t), d + 3, n))
    if len(t) == 0:
        return out
    _abi.check(lib.cssm_simulate_from(desc.ptr(), n, int(key) & _U64, xx.ctypes.data_as(_dp), int(first_step), float(t0), t.ctypes.data_as(_dp),
                                      len(t), int(rows_per_launch), int(device), out.ctypes.data_as(_dp)))
    return out


def simulate_last_ms() -> float:
    """Device time (ms) of this thread's last ``simulate`` / ``simulate_from`` (HIP events around its kernels)."""
    ms = C.c_double()
    _abi.check(_abi.load_library().cssm_simulate_last_ms(C.byref(ms)))
    return float(ms.value)


def points_of(t0: Optional[float], times, rows: np.ndarray, path: int = 0) -> List[SimulatedPoint]:
    """One path of simulated rows (``[R, d + 3, n_paths]``) as points: with ``t0`` the rows are those of ``simulate`` (R = T + 1, the first
    one at t0), with ``t0 = None`` those of ``simulate_from`` (R = T)."""
    ts = ([] if t0 is None else [float(t0)]) + [float(v) for v in times]
    if len(ts) != len(rows):
        raise ValueError(f"{len(rows)} rows for {len(ts)} times")
    d = rows.shape[1] - 3
    return [SimulatedPoint(ts[h], float(r[d + 2, path]), float(r[d + 1, path]), float(r[d, path]), r[:d, path].copy()) for h, r in enumerate(rows)]


@dataclass(frozen=True)
class LgcpSim:
    """What ``cssm_simulate_lgcp`` returns, for every path: the grid (``grid_t [G]``; ``grid [G, d + 3, n_paths]`` -- the d states, gamma,
    eta, obs = 0.0 -- or None when it was not kept) and the events in path order (path i owns ``ev_off[i] .. ev_off[i + 1] - 1``, in time
    order: ``ev_t``, the grid index ``ev_idx`` and ``ev_rows [E, d + 3]`` -- the states at that index, gamma, eta, 1.0), with the bound
    ``upper``, the ``candidates`` taken and the ``status`` (non-zero: the path was not thinned, include/cssm_obs_draws.h) per path."""
    grid_t: np.ndarray
    grid: Optional[np.ndarray]
    ev_off: np.ndarray
    ev_t: np.ndarray
    ev_idx: np.ndarray
    ev_rows: np.ndarray
    upper: np.ndarray
    candidates: np.ndarray
    status: np.ndarray

    def events(self, path: int = 0) -> List[SimulatedPoint]:
        """The events of one path in time order, each with the state of the grid point before it (observation 1.0)."""
        a, b = int(self.ev_off[path]), int(self.ev_off[path + 1])
        d = self.ev_rows.shape[1] - 3
        return [SimulatedPoint(float(self.ev_t[e]), float(r[d + 2]), float(r[d + 1]), float(r[d]), r[:d].copy())
                for e, r in zip(range(a, b), self.ev_rows[a:b])]

    def points(self, path: int = 0) -> List[SimulatedPoint]:
        """The reference's vector (Data.scala:138,144-148): the events newest first, then every grid point in time order (observation
        0.0).  Needs the grid (``keep_grid``)."""
        if self.grid is None:
            raise ValueError("the grid rows were not kept (keep_grid=False): only events() can be formed")
        return self.events(path)[::-1] + points_of(None, self.grid_t, self.grid, path)


def simulate_lgcp(model: Model, start: float, end: float, precision: int, n_paths: int = 1, key: Optional[int] = None, keep_grid: bool = True,
                  device: int = 0, paths_per_launch: int = 0) -> LgcpSim:
    """cssm_simulate_lgcp: ``n_paths`` realisations of the Cox process on ``[start, end]`` by thinning, the latent state on the grid of
    step ``10^-precision``.  ``key``: the Philox key (None: ``sim_key(20260101)``)."""
    lib = _abi.load_library()
    desc = model.descriptor()
    key = sim_key(20260101) if key is None else int(key) & _U64
    h = C.c_void_p()
    _abi.check(lib.cssm_simulate_lgcp(desc.ptr(), int(n_paths), key, float(start), float(end), int(precision),
                                      _abi.CSSM_LGCP_SIM_KEEP_GRID if keep_grid else 0, int(paths_per_launch), int(device), C.byref(h)))
    try:
        d, n, G, E = C.c_int(), C.c_uint64(), C.c_uint64(), C.c_uint64()
        _abi.check(lib.cssm_lgcp_sim_shape(h, C.byref(d), C.byref(n), C.byref(G), C.byref(E)))
        d, n, G, E = d.value, n.value, G.value, E.value
        grid_t = np.zeros(G)
        grid = np.zeros((G, d + 3, n)) if keep_grid else None
        ev_off, upper = np.zeros(n + 1, dtype=np.uint64), np.zeros(n)
        cand, status = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.int32)
        ev_t, ev_idx, ev_rows = np.zeros(E), np.zeros(E, dtype=np.uint32), np.zeros((E, d + 3))
        u64p, u32p, i32p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_int32)
        _abi.check(lib.cssm_lgcp_sim_grid_times(h, grid_t.ctypes.data_as(_dp)))
        if keep_grid:
            _abi.check(lib.cssm_lgcp_sim_grid(h, grid.ctypes.data_as(_dp)))
        _abi.check(lib.cssm_lgcp_sim_paths(h, ev_off.ctypes.data_as(u64p), upper.ctypes.data_as(_dp), cand.ctypes.data_as(u32p),
                                           status.ctypes.data_as(i32p)))
        _abi.check(lib.cssm_lgcp_sim_events(h, ev_t.ctypes.data_as(_dp), ev_idx.ctypes.data_as(u32p), ev_rows.ctypes.data_as(_dp)))
    finally:
        lib.cssm_lgcp_sim_destroy(h)
    return LgcpSim(grid_t, grid, ev_off, ev_t, ev_idx, ev_rows, upper, cand, status)


def simulate_lgcp_last_ms() -> tuple:
    """Device time (ms) of this thread's last ``simulate_lgcp``: (its grid kernels, its thinning launches)."""
    ms = (C.c_double * 2)()
    _abi.check(_abi.load_library().cssm_simulate_lgcp_last_ms(ms))
    return float(ms[0]), float(ms[1])


def lgcp_events_data(points_or_sim: Union[LgcpSim, Iterable[SimulatedPoint]], path: int = 0) -> List[TimedObservation]:
    """The events of a simulated Cox process as the data of a filter: ``TimedObservation(t, 1.0)`` in time order -- from an ``LgcpSim``
    (its path ``path``) or from the reference's vector of points (``simLGCP``: the points that observed 1.0, newest first)."""
    if isinstance(points_or_sim, LgcpSim):
        return [p.to_data() for p in points_or_sim.events(path)]
    ev = [p.to_data() for p in points_or_sim if p.observation == 1.0]
    return sorted(ev, key=lambda o: o.t)


def lgcp_fleet_data(sim: LgcpSim) -> List[np.ndarray]:
    """The events of every path of a simulated Cox process as the data of an LGCP fleet: one array of event times per path, in time
    order -- what ``filter.NativeLgcpFleet.ll_filter`` takes, series p the path p (``lgcp_events_data(sim, p)`` without the objects)."""
    off = [int(v) for v in sim.ev_off]
    return [np.ascontiguousarray(sim.ev_t[a:b], dtype=np.float64) for a, b in zip(off, off[1:])]


class SimulateData:
    """``SimulateData(model)`` of the reference (Data.scala:53-100), one path, drawn on the device under ``sim_key(seed)``."""

    BLOCK = 1024   # time indices one device call of the lazy iterators covers

    def __init__(self, model: Model, seed: int = 20260101, device: int = 0):
        self.model, self.seed, self.device = model, int(seed), int(device)
        self._key = None
        self._steps = 0   # simStep draws made so far (each takes the next step index)

    @property
    def key(self) -> int:
        if self._key is None:
            self._key = sim_key(self.seed)
        return self._key

    def _call(self, key: int, first_step: Optional[int], t0: float, x, times) -> np.ndarray:
        """The one native seam: ``first_step`` None = a simulation from the initial draw (``[T + 1, d + 3, 1]``), else one continued from the
        state ``x`` at ``t0`` under steps ``first_step ..`` (``[T, d + 3, 1]``)."""
        if first_step is None:
            return simulate(self.model, t0, times, 1, key, self.device)
        return simulate_from(self.model, x, first_step, t0, times, key, self.device)

    def _lgcp(self, key: int, start: float, end: float, precision: int) -> LgcpSim:
        """The native seam of simLGCP."""
        return simulate_lgcp(self.model, start, end, precision, 1, key, True, self.device)

    def simLGCP(self, start: float, end: float, precision: int) -> List[SimulatedPoint]:
        """Data.scala:110-149: the events on ``[start, end]`` newest first (observation 1.0), then the grid of step ``10^-precision`` in
        time order (observation 0.0).  Raises where the reference would throw or not return: a bound that is not finite, or more
        candidates than a path may take (include/cssm_obs_draws.h)."""
        sim = self._lgcp(self.key, float(start), float(end), int(precision))
        st = int(sim.status[0])
        if st != _abi.CSSM_LGCP_PATH_OK:
            what = "is not finite" if st == _abi.CSSM_LGCP_PATH_NONFINITE else "asks for more candidates than a path may take"
            raise CssmError(_abi.CSSM_ENONFINITE, f"simLGCP: the upper bound of the hazard, {float(sim.upper[0])!r}, {what} (path status {st})")
        return sim.points(0)

    def simPompModel(self, t0: float) -> Callable[[Iterable[float]], List[SimulatedPoint]]:
        """Data.scala:64-73: the point at ``t0``, then one per time (the Flow's scan emits its initial value first)."""
        def run(times: Iterable[float]) -> List[SimulatedPoint]:
            t = _times(times)
            return points_of(t0, t, self._call(self.key, None, float(t0), None, t))
        return run

    def simMarkov(self, dt: float, block: Optional[int] = None) -> Iterator[SimulatedPoint]:
        """Data.scala:81-91: the chain from t = 0 on the grid t + dt (accumulated as the reference's ``d.t + deltat`` is), lazily: the device
        simulates ``block`` time indices per call and the next call continues from the last state under the following step indices, so the
        points do not depend on the block size."""
        B = int(block or self.BLOCK)
        if B < 2:
            raise ValueError("a block holds at least two time indices")
        dt = float(dt)

        def grid(t, count):
            out = []
            for _ in range(count):
                t = t + dt
                out.append(t)
            return out

        def chain():
            times = grid(0.0, B - 1)
            pts = points_of(0.0, times, self._call(self.key, None, 0.0, None, times))
            done = B - 1     # transitions made so far = the next step index
            while True:
                yield from pts
                last = pts[-1]
                times = grid(last.t, B)
                pts = points_of(None, times, self._call(self.key, done, last.t, last.sdeState, times))
                done += B
        return chain()

    def simRegular(self, dt: float) -> Iterator[SimulatedPoint]:  # Data.scala:98-100
        return self.simMarkov(dt)

    @property
    def observations(self) -> Iterator[SimulatedPoint]:  # Data.scala:54
        return self.simRegular(0.1)

    def simStep(self, dt: float) -> Callable[..., SimulatedPoint]:
        """Data.scala:186-193: ``d -> `` one draw of the point ``dt`` after ``d``.  Every draw takes a step index of its own: ``step`` if
        given, else this object's count of draws so far."""
        def step_fn(d: SimulatedPoint, step: Optional[int] = None) -> SimulatedPoint:
            if step is None:
                step = self._steps
                self._steps += 1
            t1 = d.t + float(dt)
            return points_of(None, [t1], self._call(self.key, int(step), d.t, d.sdeState, [t1]))[0]
        return step_fn
