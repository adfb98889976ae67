"""-m gpu: SimulateData.simLGCP on the device (include/cssm_pf.h: cssm_simulate_lgcp; csrc/cssm_simulate_lgcp.hip: k_lgcp_grid,
k_lgcp_thin), anchored on what the repository already holds to the oracle:

  the grid   its times are the Python accumulation; its state rows are a chain of single-step cssm_simulate_from calls on the model's
             Poisson twin (the same leaves under Model.poisson: dt = delta exactly, the same counters), its whole rows cssm_simulate of
             that twin where the differences of the grid times are exact; row 0 is a handle's initial cloud;
  the events the host twin of the thinning statements (tests/cpp/lgcp_thin_twin.c, held to model/Data.scala:122-143 in
             tests/test_simulate_lgcp_host.py) fed the device's own eta column and bound.

Then the flagged paths, the independence of the chunking, the exact count law of thinning (no oracle), the round trip through the
filters and the Python surface."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import pytest

import cases
from composablestatespacemodels_amd import _abi, lgcp_events_data, simulate_lgcp, simulate_lgcp_last_ms
from composablestatespacemodels_amd.filter import FilterLgcp, NativePf, Resampling, split_data
from composablestatespacemodels_amd.model import Model, Parameters, Sde, SdeParameter
from composablestatespacemodels_amd.simulate import SimulateData, simulate, simulate_from
from oracle import oracle
from test_simulate_lgcp_host import GRID_TABLE, accumulate, build_lgcp_twin, twin_thin

pytestmark = pytest.mark.gpu

KEY = 0x16C9
BLOCK = 256          # CSSM_BLOCK: pairs per workgroup of k_lgcp_grid
NS = [1, 2, 5, 2 * BLOCK + 1]
_dp = C.POINTER(C.c_double)


def _ou(m0=0.1):
    return SdeParameter.ouParameter(m0, 0.5, 0.4, 0.1, 0.5)          # C4's parameters


_SEASON = SdeParameter.ouParameter(0.0, 0.3, 0.2, [0.3, -0.2], 0.2)


def models(name, m0=0.1):
    """(the Cox-process model, its Poisson twin: the same leaves, Model.poisson leftmost)"""
    if name == "L1":
        p = Parameters.apply(None, _ou(m0))
        return Model.lgcp(Sde.ouProcess(1)).run(p), Model.poisson(Sde.ouProcess(1)).run(p)
    p = Parameters.apply(None, _ou(m0)) | Parameters.apply(None, _SEASON)
    season = lambda: Model.seasonal(24, 1, Sde.ouProcess(2))
    return (Model.lgcp(Sde.ouProcess(1)) | season()).run(p), (Model.poisson(Sde.ouProcess(1)) | season()).run(p)


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    return build_lgcp_twin(tmp_path_factory.mktemp("lgcp_twin"))


@pytest.mark.parametrize("case", GRID_TABLE, ids=lambda c: "%g-%g-p%d" % c[0])
def test_grid_times_are_the_accumulation(case):
    (start, end, precision), (points, last) = case
    s = simulate_lgcp(models("L3")[0], start, end, precision, 2, KEY, keep_grid=precision < 2)
    want, _ = accumulate(start, end, precision)
    assert len(s.grid_t) == points and s.grid_t[-1] == last
    assert s.grid_t.tobytes() == want.tobytes()
    assert (s.grid is None) == (precision >= 2) and (s.grid is None or s.grid.shape == (points, 6, 2))


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("name", ["L1", "L3"])
@pytest.mark.parametrize("interval", [(0.0, 2.0, 1), (0.0, 0.5, 2)], ids=["p1", "p2"])
def test_states_are_a_chain_of_single_steps_of_the_poisson_twin(interval, name, n):
    """Every transition takes dt = delta exactly (not t_k - t_(k-1), which rounding moves) under step k - 1: grid index k is ONE
    cssm_simulate_from step of the Poisson twin from t0 = 0 to t = delta, from the row before.  With a constant f (L1) gamma and eta are
    that step's too; row 0 is the initial cloud of a handle of n particles under the key."""
    start, end, precision = interval
    lgcp, pois = models(name)
    s = simulate_lgcp(lgcp, start, end, precision, n, KEY)
    d = s.grid.shape[1] - 3
    delta = math.pow(10, -precision)
    with NativePf(pois, n, cases.SEED) as g:
        g.reseed(KEY)
        g.init(start)
        assert np.array_equal(s.grid[0, :d], g.particles())
    rows = d + 2 if name == "L1" else d
    x = s.grid[0, :d]
    for k in range(1, len(s.grid_t)):
        step = simulate_from(pois, x, k - 1, 0.0, [delta], KEY)[0]
        assert np.array_equal(s.grid[k, :rows], step[:rows]), k
        x = step[:d]
    assert np.all(s.grid[:, d + 2] == 0.0)


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("name", ["L1", "L3"])
@pytest.mark.parametrize("interval", [(0.0, 6.0), (2.0, 8.0)], ids=["0-6", "2-8"])
def test_whole_rows_are_the_poisson_twins_simulation(interval, name, n):
    """delta = 1.0: the differences of the grid times are exact, so cssm_simulate of the Poisson twin over the grid times makes the same
    transitions and evaluates the same (time-dependent) f: states, gamma and eta bit for bit."""
    start, end = interval
    lgcp, pois = models(name)
    s = simulate_lgcp(lgcp, start, end, 0, n, KEY)
    d = s.grid.shape[1] - 3
    assert len(s.grid_t) == 7 and np.array_equal(s.grid_t, start + np.arange(7.0))
    want = simulate(pois, start, s.grid_t[1:], n, KEY)
    assert np.array_equal(s.grid[:, :d + 2], want[:, :d + 2])
    assert np.all(s.grid[:, d + 2] == 0.0)
    assert np.array_equal(s.upper, s.grid[:, d + 1].max(axis=0))
    if name == "L3":
        assert not np.array_equal(s.grid[:, d], s.grid[:, 0])       # f depends on the seasonal states and the time


def lgcp_dim_model(d):
    """cases.dim_model(d) with Model.lgcp leftmost: lgcp(ou(1 or 2)) |+| seasonal(24, h, ou(2 h)), the same parameters."""
    first = 1 if d % 2 else 2
    p = Parameters.apply(None, SdeParameter.ouParameter(0.0, 0.5, 0.2, [0.1, -0.05][:first], 0.2))
    m = Model.lgcp(Sde.ouProcess(first))
    h = (d - first) // 2
    if h:
        p = p | Parameters.apply(None, SdeParameter.ouParameter(0.0, 0.2, 0.2, [0.05 * ((i % 3) - 1) for i in range(2 * h)], 0.1))
        m = m | Model.seasonal(24, h, Sde.ouProcess(2 * h))
    return m.run(p)


@pytest.mark.parametrize("d", range(1, 17))
def test_every_latent_dimension(d, twin):
    """k_lgcp_grid<D> at every D: the rows of cases.dim_model(d) (the Poisson twin) over the grid of delta = 1.0, and the thinning on
    them -- 3 paths: a pair and the unpaired last one."""
    start, end, n = 0.0, 6.0, 3
    s = simulate_lgcp(lgcp_dim_model(d), start, end, 0, n, KEY + d)
    assert s.grid.shape == (7, d + 3, n)
    want = simulate(cases.dim_model(d), start, s.grid_t[1:], n, KEY + d)
    assert np.array_equal(s.grid[:, :d + 2], want[:, :d + 2]) and np.all(s.grid[:, d + 2] == 0.0)
    assert np.array_equal(s.upper, s.grid[:, d + 1].max(axis=0))
    for i in range(n):
        st, ev_t, ev_idx, nc = twin_thin(twin, KEY + d, i, s.grid_t, s.grid[:, d + 1, i], start, end, 1.0, float(s.upper[i]))
        a, b = int(s.ev_off[i]), int(s.ev_off[i + 1])
        assert s.status[i] == st == 0 and s.candidates[i] == nc
        assert np.array_equal(s.ev_t[a:b], ev_t) and np.array_equal(s.ev_idx[a:b], ev_idx)
        assert all(np.array_equal(s.ev_rows[e, :d + 2], s.grid[s.ev_idx[e], :d + 2, i]) and s.ev_rows[e, d + 2] == 1.0 for e in range(a, b))


THIN_CASES = {"L1": ("L1", 0.1), "L3": ("L3", 0.1), "hot": ("L1", 2.5), "cold": ("L1", -30.0)}


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("case", list(THIN_CASES))
def test_thinning_is_the_twins_loop_on_the_devices_own_grid(case, n, twin):
    name, m0 = THIN_CASES[case]
    start, end, precision = 0.0, 2.0, 1
    s = simulate_lgcp(models(name, m0)[0], start, end, precision, n, KEY)
    d = s.grid.shape[1] - 3
    delta = math.pow(10, -precision)
    assert np.array_equal(s.upper, s.grid[:, d + 1].max(axis=0))
    assert s.ev_off[0] == 0 and len(s.ev_off) == n + 1 and s.ev_off[-1] == len(s.ev_t) == len(s.ev_idx) == len(s.ev_rows)
    counts = []
    for i in range(n):
        st, ev_t, ev_idx, nc = twin_thin(twin, KEY, i, s.grid_t, s.grid[:, d + 1, i], start, end, delta, float(s.upper[i]))
        a, b = int(s.ev_off[i]), int(s.ev_off[i + 1])
        assert s.status[i] == st == 0 and s.candidates[i] == nc, i
        assert np.array_equal(s.ev_t[a:b], ev_t) and np.array_equal(s.ev_idx[a:b], ev_idx), i
        assert np.all(np.diff(s.ev_t[a:b]) >= 0.0) and (a == b or s.ev_t[b - 1] <= end), i
        for e in range(a, b):
            assert np.array_equal(s.ev_rows[e, :d + 2], s.grid[s.ev_idx[e], :d + 2, i]) and s.ev_rows[e, d + 2] == 1.0
        counts.append(b - a)
    assert np.array_equal(s.ev_off, np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64))   # the exclusive scan, in path order
    if case == "hot" and n > 2:
        assert s.candidates.mean() > 10.0 and sum(counts) > n          # (about 25 candidates per path)
    if case == "cold":
        assert sum(counts) == 0 and len(s.ev_t) == 0
    assert simulate_lgcp_last_ms()[0] > 0.0 and simulate_lgcp_last_ms()[1] > 0.0


@pytest.mark.parametrize("n", [1, 5])
def test_a_path_that_would_take_too_many_candidates_is_flagged_and_left(n):
    """m0 = 40: ub (end - start) is far above 2^20, the path takes no candidate -- an early exit, the call succeeds."""
    s = simulate_lgcp(models("L1", 40.0)[0], 0.0, 2.0, 1, n, KEY)
    assert np.all(s.status == _abi.CSSM_LGCP_PATH_TOO_MANY) and np.all(s.candidates == 0) and len(s.ev_t) == 0 and np.all(s.ev_off == 0)
    assert np.all(np.isfinite(s.upper)) and np.all(s.upper * 2.0 > 2.0**20)
    with pytest.raises(_abi.CssmError, match="more candidates"):
        SimulateData(models("L1", 40.0)[0], seed=3).simLGCP(0.0, 2.0, 1)


def test_the_chunking_does_not_show():
    lgcp = models("L3", 1.5)[0]
    want = simulate_lgcp(lgcp, 0.0, 2.0, 1, 5, KEY)
    assert len(want.ev_t) > 5
    for ppl in (0, 2, 3):
        for keep in (True, False):
            s = simulate_lgcp(lgcp, 0.0, 2.0, 1, 5, KEY, keep_grid=keep, paths_per_launch=ppl)
            for f in ("grid_t", "ev_off", "ev_t", "ev_idx", "ev_rows", "upper", "candidates", "status"):
                assert np.array_equal(getattr(s, f), getattr(want, f)), (ppl, keep, f)
            assert (s.grid is None) if not keep else np.array_equal(s.grid, want.grid), (ppl, keep)
    # the grid rows of a call that did not keep them: CSSM_ESTATE
    lib = _abi.load_library()
    h = C.c_void_p()
    _abi.check(lib.cssm_simulate_lgcp(lgcp.descriptor().ptr(), 5, KEY, 0.0, 2.0, 1, 0, 0, 0, C.byref(h)))
    try:
        buf = np.full((20, 6, 5), -7.0)
        assert lib.cssm_lgcp_sim_grid(h, buf.ctypes.data_as(_dp)) == _abi.CSSM_ESTATE and "not kept" in _abi.last_error()
        assert np.all(buf == -7.0)
        E = C.c_uint64()
        _abi.check(lib.cssm_lgcp_sim_shape(h, None, None, None, C.byref(E)))
        assert E.value == len(want.ev_t)
    finally:
        lib.cssm_lgcp_sim_destroy(h)


def test_the_count_law_of_thinning():
    """Conditional on its grid, the events of a path are a Poisson process of the piecewise constant rate eta_k on [t_k, t_(k+1)) (the
    last cell runs to `end`), so its count is Poisson with mean Lambda_i = sum_k eta_k,i (min(t_(k+1), end) - t_k); the counts of
    independent paths add up: sum_i (count_i - Lambda_i) has mean 0 and variance sum_i Lambda_i.  Five standard deviations: a correct
    implementation fails with probability below 1e-6 (and under a fixed key the outcome is fixed)."""
    n, start, end = 4096, 0.0, 2.0
    s = simulate_lgcp(models("L1")[0], start, end, 1, n, KEY)
    eta = s.grid[:, 2]
    width = np.diff(np.append(s.grid_t, end))
    lam = (eta * width[:, None]).sum(axis=0)
    counts = np.diff(s.ev_off.astype(np.int64))
    print("sum(count - Lambda) =", float((counts - lam).sum()), " bound =", 5.0 * math.sqrt(lam.sum()), " events =", int(counts.sum()))
    assert np.all(s.status == 0)
    assert abs(float((counts - lam).sum())) <= 5.0 * math.sqrt(float(lam.sum()))


def test_round_trip_the_filters_take_the_events_the_model_produced():
    lgcp = models("L1", 2.5)[0]
    s = simulate_lgcp(lgcp, 0.0, 2.0, 1, 8, KEY)
    path = int(np.argmax(np.diff(s.ev_off.astype(np.int64))))
    data = lgcp_events_data(s, path)
    assert len(data) >= 5 and all(d.observation == 1.0 for d in data) and [d.t for d in data] == sorted(d.t for d in data)
    t, y, has = split_data(data)
    n = 512
    with NativePf(lgcp, n, cases.SEED, lgcp_precision=1) as g:
        gl = g.run(t, y, has)[0]
    ol = oracle.OraclePf(lgcp.descriptor(1), n, cases.SEED).filter(t, y, has)[0]
    fl = FilterLgcp(lgcp, Resampling.systematicResampling, 1, seed=cases.SEED).llFilter(data, n)
    assert math.isfinite(gl) and gl == ol and fl == ol, (gl, fl, ol)


def test_sim_lgcp_returns_the_references_vector():
    lgcp = models("L1", 1.0)[0]
    sd = SimulateData(lgcp, seed=7)
    pts = sd.simLGCP(0, 2, 1)
    ev = [p for p in pts if p.observation == 1.0]
    grid = pts[len(ev):]
    assert len(ev) >= 1 and len(grid) == 20 and all(p.observation == 0.0 for p in grid) and all(p.observation == 1.0 for p in pts[:len(ev)])
    assert grid[0].t == 0.0 and [p.t for p in grid] == list(accumulate(0.0, 2.0, 1)[0])
    assert [p.t for p in ev] == sorted((p.t for p in ev), reverse=True) and ev[0].t <= 2.0       # newest first
    for p in ev:                                                      # an event carries the grid point before it
        k = max(j for j, q in enumerate(grid) if q.t <= p.t)
        assert (p.eta, p.gamma) == (grid[k].eta, grid[k].gamma) and np.array_equal(p.sdeState, grid[k].sdeState)
    assert all(p.eta == math.exp(p.gamma) or abs(p.eta - math.exp(p.gamma)) <= 1e-15 * p.eta for p in grid)
    again = SimulateData(lgcp, seed=7).simLGCP(0, 2, 1)
    assert [(p.t, p.observation, p.eta) for p in again] == [(p.t, p.observation, p.eta) for p in pts]
    other = SimulateData(lgcp, seed=8).simLGCP(0, 2, 1)
    assert [p.eta for p in other[-20:]] != [p.eta for p in grid]
    assert lgcp_events_data(pts) == [p.to_data() for p in ev[::-1]]
    sim = simulate_lgcp(lgcp, 0.0, 2.0, 1, 1, sd.key)
    assert [p.t for p in sim.points(0)] == [p.t for p in pts]
