"""CPU-only checks of SimulateData.simLGCP's host side (include/cssm_pf.h: cssm_simulate_lgcp and its result object): the ctypes view
against the header, every refusal that is decided before the first device call returned without a device, the thinning statements of
include/cssm_obs_draws.h (their host twin, tests/cpp/lgcp_thin_twin.c) against a restatement of model/Data.scala:122-143 written here,
the pure Python of composablestatespacemodels_amd/simulate.py (LgcpSim's splitting and ordering, lgcp_events_data, simLGCP over a
recording stub), and the host plan as a stand-alone program under sanitizers."""
from __future__ import annotations

import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import cases
from composablestatespacemodels_amd import _abi, formats as F
from composablestatespacemodels_amd import CssmError, LgcpSim, lgcp_events_data
from composablestatespacemodels_amd.model import Model, Parameters, Sde, SdeParameter, TimedObservation
from composablestatespacemodels_amd.simulate import SimulateData

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEY = 0x16C9
_dp = C.POINTER(C.c_double)
_u32p = C.POINTER(C.c_uint32)

# the table of the grid: (start, end, precision) -> (grid points, last grid time)
GRID_TABLE = (((0.0, 0.3, 1), (3, 0.2)), ((0.0, 1.0, 1), (11, 0.9999999999999999)), ((0.0, 2.0, 1), (20, 1.9000000000000006)),
              ((0.5, 2.5, 1), (20, 2.400000000000001)), ((0.0, 0.5, 2), (50, 0.49000000000000027)), ((0.0, 6.0, 0), (7, 6.0)),
              ((0.0, 10.0, 2), (1001, 9.999999999999831)))


def accumulate(start, end, precision):
    """simSdeStream's times (model/Data.scala:169-175): t + delta by repeated addition while t <= start + (end - start)."""
    delta = math.pow(10, -precision)
    t, out = start, []
    while t <= start + (end - start):
        out.append(t)
        t = t + delta
    return np.array(out), delta


def build_lgcp_twin(out_dir) -> C.CDLL:
    so = os.path.join(str(out_dir), "lgcp_thin_twin.so")
    subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-mfma", "-std=c99", "-shared", "-fPIC", "-o", so,
                           os.path.join(ROOT, "tests", "cpp", "lgcp_thin_twin.c"), "-lm"])
    lib = C.CDLL(so)
    lib.twin_lgcp_candidate.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32, C.c_double, _dp, _dp]
    lib.twin_lgcp_candidate.restype = None
    lib.twin_lgcp_index.argtypes = [_dp, C.c_uint32, C.c_double, C.c_double, C.c_double]
    lib.twin_lgcp_index.restype = C.c_uint32
    lib.twin_lgcp_thin.argtypes = [C.c_uint64, C.c_uint64, _dp, _dp, C.c_uint32, C.c_double, C.c_double, C.c_double, C.c_double, _dp, _u32p,
                                   C.c_size_t, _u32p, _u32p]
    lib.twin_lgcp_thin.restype = C.c_int
    return lib


def twin_thin(twin, key, i, grid_t, eta, start, end, delta, ub, cap=4096):
    """(status, event times, event grid indices, candidates) of path i from its eta column."""
    grid_t, eta = np.ascontiguousarray(grid_t, dtype=np.float64), np.ascontiguousarray(eta, dtype=np.float64)
    ev_t, ev_idx = np.zeros(cap), np.zeros(cap, dtype=np.uint32)
    ne, nc = C.c_uint32(), C.c_uint32()
    st = twin.twin_lgcp_thin(key, i, grid_t.ctypes.data_as(_dp), eta.ctypes.data_as(_dp), len(grid_t), start, end, delta, ub,
                             ev_t.ctypes.data_as(_dp), ev_idx.ctypes.data_as(_u32p), cap, C.byref(ne), C.byref(nc))
    assert ne.value <= cap
    return st, ev_t[:ne.value], ev_idx[:ne.value], nc.value


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    return build_lgcp_twin(tmp_path_factory.mktemp("lgcp_twin"))


def test_the_header_declares_what_the_ctypes_view_binds():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cssm_pf.h")).read(), flags=re.S)
    bound = {n: (res, args) for n, res, args in _abi.SYMBOLS}
    for name, nargs in (("cssm_simulate_lgcp", 10), ("cssm_lgcp_sim_shape", 5), ("cssm_lgcp_sim_grid_times", 2), ("cssm_lgcp_sim_grid", 2),
                        ("cssm_lgcp_sim_paths", 5), ("cssm_lgcp_sim_events", 4), ("cssm_simulate_lgcp_last_ms", 1)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", src)
        assert m and len(m.group(1).split(",")) == nargs == len(bound[name][1]), name
        assert hasattr(_abi.load_library(), name)
    m = re.search(r"\bvoid\s+cssm_lgcp_sim_destroy\s*\(([^;]*?)\)\s*;", src)
    assert m and len(m.group(1).split(",")) == 1 == len(bound["cssm_lgcp_sim_destroy"][1]) and bound["cssm_lgcp_sim_destroy"][0] is None
    assert re.search(r"#define CSSM_LGCP_SIM_KEEP_GRID 1\b", src) and _abi.CSSM_LGCP_SIM_KEEP_GRID == 1
    draws = open(os.path.join(ROOT, "include", "cssm_obs_draws.h")).read()
    tags = {int(v) for v in re.findall(r"#define CSSM_STREAM_\w+ (\d+)u", draws + open(os.path.join(ROOT, "include", "cssm_numerics.h")).read())}
    assert re.search(r"#define CSSM_STREAM_THIN 10u", draws) and _abi.CSSM_STREAM_THIN == 10 and tags == set(range(11))   # the next free tag
    assert re.search(r"#define CSSM_LGCP_MAX_EXPECTED 0x1\.0p20", draws) and re.search(r"#define CSSM_LGCP_MAX_CANDIDATES \(1u << 21\)", draws)
    for name, v in (("OK", 0), ("NONFINITE", 1), ("TOO_MANY", 2)):
        assert re.search(r"#define CSSM_LGCP_PATH_%s %d\b" % (name, v), draws) and getattr(_abi, "CSSM_LGCP_PATH_" + name) == v


def _raw(desc, n, start, end, precision, flags=1, device=10000, null_out=False):
    lib = _abi.load_library()
    h = C.c_void_p()
    rc = lib.cssm_simulate_lgcp(None if desc is None else desc.ptr(), n, KEY, float(start), float(end), precision, flags, 0, device,
                                None if null_out else C.byref(h))
    return rc, _abi.last_error(), h.value


def test_refusals_come_before_any_device_call_and_leave_the_result_slot_null():
    """Device 10 000 does not exist anywhere: a refusal that names its own cause was made before the device was looked at."""
    l1 = cases.c4_model().descriptor(2)
    l3 = cases.lgcp_seasonal_model().descriptor(2)
    poisson = cases.c2_model().descriptor()
    bad_prec = cases.c4_model().descriptor(12)          # the descriptor's own precision: validated though the call's rules
    nan, inf = float("nan"), float("inf")
    A, D = _abi.CSSM_EINVAL_ARG, _abi.CSSM_EINVAL_DESC
    for args, code, word in (((None, 2, 0.0, 1.0, 1), A, "null argument"),
                             ((l1, 0, 0.0, 1.0, 1), A, "n_paths"),
                             ((l1, 2**32 - 2**16 + 1, 0.0, 1.0, 1), A, "n_paths"),
                             ((l1, 2, 0.0, 1.0, -1), A, "precision"),
                             ((l1, 2, 0.0, 1.0, 10), A, "precision"),
                             ((l1, 2, nan, 1.0, 1), A, "start is not finite"),
                             ((l1, 2, 0.0, inf, 1), A, "end is not finite"),
                             ((l1, 2, 1.0, 0.5, 1), A, "is before start"),
                             ((poisson, 2, 0.0, 1.0, 1), A, "cssm_simulate"),
                             ((bad_prec, 2, 0.0, 1.0, 1), D, "lgcp_precision"),
                             ((l1, 2, 0.0, 100.0, 9), A, "too many grid points"),
                             ((l3, 2, 0.0, 1.2e7, 0), A, "exceed the 1 GiB"),
                             ((l1, 2, 0.0, 1.0, 1, 6), A, "unknown flags")):
        rc, msg, h = _raw(*args)
        assert rc == code and word in msg, (word, rc, msg)
        assert h is None, word
    rc, msg, _ = _raw(l1, 2, 0.0, 1.0, 1, null_out=True)
    assert rc == A and "null argument" in msg
    # an accepted call reaches the device, and only then fails; the slot stays null
    rc, msg, h = _raw(l1, 2, 0.0, 1.0, 1)
    assert rc in (_abi.CSSM_EHIP, _abi.CSSM_EINVAL_ARG) and ("device" in msg or "HIP" in msg) and h is None, msg
    # the result object's readers refuse a null object; destroying null is allowed
    lib = _abi.load_library()
    for call in (lambda: lib.cssm_lgcp_sim_shape(None, None, None, None, None), lambda: lib.cssm_lgcp_sim_grid_times(None, None),
                 lambda: lib.cssm_lgcp_sim_grid(None, None), lambda: lib.cssm_lgcp_sim_paths(None, None, None, None, None),
                 lambda: lib.cssm_lgcp_sim_events(None, None, None, None), lambda: lib.cssm_simulate_lgcp_last_ms(None)):
        assert call() == A and "null argument" in _abi.last_error()
    lib.cssm_lgcp_sim_destroy(None)
    # cssm_simulate keeps refusing the model, in the words it had
    out = np.zeros((2, 4, 1))
    t = np.array([1.0])
    assert lib.cssm_simulate(l1.ptr(), 1, KEY, 0.0, t.ctypes.data_as(_dp), 1, 0, 10000, out.ctypes.data_as(_dp)) == A
    assert "log-Gaussian Cox" in _abi.last_error()


def test_the_grid_of_the_table_in_python():
    """What the accumulation yields (the lengths and last times every layer is held to) -- and that a difference of accumulated times is
    not delta, which is why the transitions take delta itself."""
    for (start, end, precision), (points, last) in GRID_TABLE:
        t, delta = accumulate(start, end, precision)
        assert len(t) == points and t[-1] == last and t[0] == start
    t, delta = accumulate(0.0, 10.0, 2)
    off = np.abs(np.diff(t) - delta)
    assert 0.0 < off.max() <= 2.0**-50      # (about 2.3e-16 here; half an ulp of a time below 16 bounds it)
    assert abs(t[-1] - 10.0) > 1e-13     # the drift of the accumulated grid from start + k delta


# ---- the thinning: the twin against Data.scala:122-143 restated

def candidate(twin, key, i, c, ub):
    E, V = C.c_double(), C.c_double()
    twin.twin_lgcp_candidate(key, i, c, ub, C.byref(E), C.byref(V))
    return E.value, V.value


def restated(twin, key, i, grid_t, eta, start, end, ub):
    """`loop` of simLGCP with (E, V) of every candidate given: ([(t1, k)] of the events oldest first, [t1] of all candidates)."""
    events, cands, last, c = [], [], start, 0
    while True:
        E, V = candidate(twin, key, i, c, ub)
        t1 = last + E                                               # lastEvent + Exponential(upperBound).draw
        if t1 > end:
            return events, cands
        c += 1
        k = [j for j, tj in enumerate(grid_t) if tj <= t1][-1]      # stateSpace.takeWhile(s => s.time <= t1).last
        if V <= eta[k] / ub:                                        # Uniform(0,1).draw <= exp(hazardt1) / upperBound
            events.append((t1, k))
        cands.append(t1)
        last = t1


def eta_column(n, seed):
    rng = np.random.default_rng(seed)
    return np.exp(rng.normal(0.0, 1.0, n))


def test_candidates_are_the_contracts_block(twin):
    E, V = candidate(twin, KEY, 7, 3, 2.5)
    assert 0.0 <= V < 1.0 and E > 0.0
    assert (E, V) == candidate(twin, KEY, 7, 3, 2.5) and (E, V) != candidate(twin, KEY, 7, 4, 2.5) and (E, V) != candidate(twin, KEY, 8, 3, 2.5)
    E2, V2 = candidate(twin, KEY, 7, 3, 5.0)
    assert V2 == V and E2 == pytest.approx(E / 2.0, rel=1e-15)      # E = -log(U) / ub, V from the other two words
    assert candidate(twin, KEY, 7, 3, 0.0)[0] == float("inf")       # every exp underflowed: no candidate


def test_the_index_rule_at_every_cell_edge(twin):
    """The largest k with t_k <= t1, at t1 = t_k itself, just below and just above, on the accumulated grid whose drift makes the
    guess floor((t1 - start) / delta) alone wrong at edges."""
    wrong_guess = 0
    for (start, end, precision), _ in GRID_TABLE:
        t, delta = accumulate(start, end, precision)
        idx = lambda t1: twin.twin_lgcp_index(t.ctypes.data_as(_dp), len(t), start, delta, t1)
        for k, tk in enumerate(t):
            assert idx(tk) == k
            assert idx(np.nextafter(tk, np.inf)) == k
            if k:
                assert idx(np.nextafter(tk, -np.inf)) == k - 1
            wrong_guess += int(min(max(math.floor((tk - start) / delta), 0), len(t) - 1) != k)
        assert idx(end) == len(t) - 1 and idx(0.5 * (t[-1] + end)) == len(t) - 1      # (t_G, end] belongs to the last grid point
    assert wrong_guess > 0


def test_the_twin_runs_the_reference_loop(twin):
    # plain columns on accumulated grids, several paths each: events, indices, candidate counts
    seen_tail = 0
    for (start, end, precision), scale in (((0.0, 2.0, 1), 30.0), ((0.5, 2.5, 1), 8.0), ((0.0, 0.5, 2), 40.0), ((0.0, 6.0, 0), 3.0)):
        t, delta = accumulate(start, end, precision)
        for i in range(6):
            eta = scale * eta_column(len(t), 100 * precision + i) / 3.0
            ub = float(eta.max())
            st, ev_t, ev_idx, nc = twin_thin(twin, KEY, i, t, eta, start, end, delta, ub)
            events, cands = restated(twin, KEY, i, t, eta, start, end, ub)
            assert st == 0 and nc == len(cands)
            assert [float(v) for v in ev_t] == [e[0] for e in events] and [int(v) for v in ev_idx] == [e[1] for e in events]
            assert len(events) > 0 and all(a <= b for a, b in zip(ev_t, ev_t[1:])) and (len(ev_t) == 0 or ev_t[-1] <= end)
            seen_tail += sum(1 for (t1, k) in events if t1 > t[-1])
            assert all(k == len(t) - 1 for (t1, k) in events if t1 > t[-1])
    assert seen_tail > 0                                             # events in (t_G, end]: they take the last grid point


def test_a_candidate_exactly_on_a_grid_time(twin):
    """The first candidate of a path lands ON a grid time (the grid point nearest to it is moved there): it sees that point, not the one
    before it."""
    start, end, ub = 0.0, 2.0, 2.0
    t0, delta = accumulate(start, end, 1)
    hits = 0
    for i in range(12):
        E0, V0 = candidate(twin, KEY, i, 0, ub)
        k = int(round(E0 / delta))
        if not 1 <= k < len(t0) - 1:
            continue
        t = t0.copy()
        t[k] = start + E0
        assert t[k - 1] < t[k] < t[k + 1]
        eta = np.full(len(t), 1e-9)
        eta[k] = ub                                                  # accepted iff it reads grid point k (V <= 1), refused at k - 1
        eta[0] = ub
        st, ev_t, ev_idx, nc = twin_thin(twin, KEY, i, t, eta, start, end, delta, ub)
        events, cands = restated(twin, KEY, i, t, eta, start, end, ub)
        assert st == 0 and nc == len(cands) and cands[0] == t[k]
        assert [float(v) for v in ev_t] == [e[0] for e in events] and [int(v) for v in ev_idx] == [e[1] for e in events]
        assert events[0] == (t[k], k)
        hits += 1
    assert hits >= 6


def test_paths_without_candidates(twin):
    start, end = 0.0, 2.0
    t, delta = accumulate(start, end, 1)
    # ub == 0: E = inf, no candidate, no special case
    st, ev_t, _, nc = twin_thin(twin, KEY, 0, t, np.zeros(len(t)), start, end, delta, 0.0)
    assert (st, len(ev_t), nc) == (_abi.CSSM_LGCP_PATH_OK, 0, 0)
    assert restated(twin, KEY, 0, t, np.zeros(len(t)), start, end, 0.0) == ([], [])
    # flagged paths: ub (end - start) above 2^20 or not finite -- no candidate is taken (the reference would not return, or throw)
    for ub, want in ((2.0**19 + 1.0, _abi.CSSM_LGCP_PATH_TOO_MANY), (math.exp(40.0), _abi.CSSM_LGCP_PATH_TOO_MANY),
                     (float("inf"), _abi.CSSM_LGCP_PATH_NONFINITE), (float("nan"), _abi.CSSM_LGCP_PATH_NONFINITE)):
        st, ev_t, _, nc = twin_thin(twin, KEY, 0, t, np.full(len(t), ub), start, end, delta, ub)
        assert (st, len(ev_t), nc) == (want, 0, 0), ub
    st, _, _, nc = twin_thin(twin, KEY, 0, t, np.full(len(t), 1e-300), start, end, delta, 2.0**19)      # exactly 2^20: admitted
    assert st == _abi.CSSM_LGCP_PATH_OK and nc > 2**19
    # an empty interval: the grid is its one point, the first candidate is after `end` (almost surely)
    st, ev_t, _, nc = twin_thin(twin, KEY, 0, t[:1], np.ones(1), 0.0, 0.0, delta, 1.0)
    assert (st, len(ev_t), nc) == (0, 0, 0)


# ---- the Python surface

def _sim(n=3, d=2, G=4, counts=(2, 0, 3)):
    grid_t = np.array([0.5 + 0.25 * g for g in range(G)])
    grid = np.arange(G * (d + 3) * n, dtype=np.float64).reshape(G, d + 3, n)
    grid[:, d + 2] = 0.0
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    E = int(off[-1])
    ev_t = np.array([0.6, 1.1, 0.55, 0.9, 1.2])[:E]
    ev_idx = np.array([0, 2, 0, 1, 2], dtype=np.uint32)[:E]
    owner = np.repeat(np.arange(n), counts)
    ev_rows = np.array([np.append(grid[ev_idx[e], :d + 2, owner[e]], 1.0) for e in range(E)])
    return LgcpSim(grid_t, grid, off, ev_t, ev_idx, ev_rows, np.full(n, 9.0), np.array([4, 1, 7], dtype=np.uint32), np.zeros(n, dtype=np.int32))


def test_lgcp_sim_splits_and_orders_its_points():
    s = _sim()
    d = 2
    ev = s.events(2)
    assert [p.t for p in ev] == [0.55, 0.9, 1.2] and all(p.observation == 1.0 for p in ev)
    for p, k in zip(ev, (0, 1, 2)):
        assert np.array_equal(p.sdeState, s.grid[k, :d, 2]) and (p.gamma, p.eta) == (s.grid[k, d, 2], s.grid[k, d + 1, 2])
    assert s.events(1) == []
    pts = s.points(0)                                                # the reference's vector: events newest first, then the grid
    assert [p.t for p in pts] == [1.1, 0.6, 0.5, 0.75, 1.0, 1.25] and [p.observation for p in pts] == [1.0, 1.0, 0.0, 0.0, 0.0, 0.0]
    assert np.array_equal(pts[3].sdeState, s.grid[1, :d, 0]) and pts[3].eta == s.grid[1, d + 1, 0] and pts[3].gamma == s.grid[1, d, 0]
    assert len(s.points(1)) == 4
    pts[0].sdeState[0] = -1.0
    assert s.ev_rows[1, 0] != -1.0                                   # a point owns its state
    nogrid = LgcpSim(s.grid_t, None, s.ev_off, s.ev_t, s.ev_idx, s.ev_rows, s.upper, s.candidates, s.status)
    assert [p.t for p in nogrid.events(0)] == [0.6, 1.1]
    with pytest.raises(ValueError, match="not kept"):
        nogrid.points(0)
    # the filter's data: the events in time order, from the object or from the reference's vector
    want = [TimedObservation(0.6, 1.0), TimedObservation(1.1, 1.0)]
    assert lgcp_events_data(s) == want and lgcp_events_data(pts) == want and lgcp_events_data(s, 1) == [] and len(lgcp_events_data(s, path=2)) == 3
    # the writers take such points as they are
    assert F.simulated_csv(ev[0]).startswith("0.55, 1.0, ") and F.simulated_from_csv(F.simulated_csv(pts[2])).observation == 0.0
    assert F.simulated_from_json(F.simulated_to_json(ev[0], [2])).t == 0.55


class _Stub(SimulateData):
    """SimulateData whose native seam of simLGCP records what it is asked for."""

    def __init__(self, status=0):
        super().__init__(cases.c4_model(), seed=11)
        self._key = 0xABCDEF
        self.calls = []
        self.status = status

    def _lgcp(self, key, start, end, precision):
        self.calls.append((key, start, end, precision))
        s = _sim()
        st = s.status.copy()
        st[0] = self.status
        return LgcpSim(s.grid_t, s.grid, s.ev_off, s.ev_t, s.ev_idx, s.ev_rows, s.upper, s.candidates, st)


def test_sim_lgcp_asks_for_one_path_under_the_objects_key():
    s = _Stub()
    pts = s.simLGCP(0, 2, 1)
    assert s.calls == [(0xABCDEF, 0.0, 2.0, 1)] and isinstance(s.calls[0][1], float)
    assert [p.t for p in pts] == [1.1, 0.6, 0.5, 0.75, 1.0, 1.25]
    for status, word in ((_abi.CSSM_LGCP_PATH_NONFINITE, "not finite"), (_abi.CSSM_LGCP_PATH_TOO_MANY, "more candidates")):
        with pytest.raises(CssmError, match=word):
            _Stub(status).simLGCP(0, 2, 1)


def test_the_host_plan_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """csrc/cssm_simulate_lgcp_plan.cpp (every refusal, the grid of the table point for point, the coefficients) over csrc/cssm_model.cpp
    as a stand-alone program with its own main (tests/cpp/lgcp_plan_main.cpp), built with -fsanitize=address,undefined and run here:
    host code, no device, nothing preloaded."""
    csrc = os.path.join(ROOT, "composablestatespacemodels_amd", "csrc")
    exe = str(tmp_path / "lgcp_plan_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-mfma", "-Wall", "-Werror", "-fno-omit-frame-pointer",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + csrc, "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "lgcp_plan_main.cpp"), os.path.join(csrc, "cssm_simulate_lgcp_plan.cpp"),
                           os.path.join(csrc, "cssm_model.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "lgcp_plan: ok" in r.stdout, r.stdout + r.stderr
