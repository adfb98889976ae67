"""CPU-only checks of the single handle's streaming interpolation (include/cssm_pf.h: cssm_pf_window, cssm_pf_window_depth,
cssm_pf_step_interpolate, cssm_pf_step_interpolate_last_ms):

  * the bindings against the header and the refusals made before a device is looked at;
  * the sequential twin of the ring (tests/cpp/window_twin.c, written on the bookkeeping the host uses:
    composablestatespacemodels_amd/csrc/cssm_window.h) against a small Python model, over seeded sequences of open / put / restart /
    re-open: the depth, the slot of every row, and that no row is read from a slot written since;
  * what NativePf and FilterInterpolate hand to the calls and make of the rows, against a recording stub; the counted budget of a row."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import cases
from composablestatespacemodels_amd import Data, _abi, load_library
from composablestatespacemodels_amd.filter import CredibleInterval, FilterInterpolate, NativePf, PfOut, Resampling
from test_filter_intervals_host import twin_constants

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_dp, _u32p = C.POINTER(C.c_double), C.POINTER(C.c_uint32)
NONE = 0xFFFFFFFF
_TWIN = None
NAMES = ("cssm_pf_window", "cssm_pf_window_depth", "cssm_pf_step_interpolate", "cssm_pf_step_interpolate_last_ms")


def build_window_twin() -> C.CDLL:
    """tests/cpp/window_twin.c built with the gcc line of the other twins (once per process)."""
    global _TWIN
    if _TWIN is None:
        so = os.path.join(tempfile.mkdtemp(prefix="window_twin_"), "window_twin.so")
        subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-mfma", "-std=c99", "-shared", "-fPIC", "-o", so,
                               os.path.join(ROOT, "tests", "cpp", "window_twin.c"), "-lm"])
        lib = C.CDLL(so)
        lib.twin_window_run.argtypes = [_u32p, _u32p, C.c_size_t, C.c_uint32, _u32p, _u32p, _u32p]
        lib.twin_window_run.restype = C.c_int
        lib.twin_window_rows.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32]
        lib.twin_window_rows.restype = C.c_uint32
        _TWIN = lib
    return _TWIN


def twin_run(events, max_rows):
    """(rc, depth[E], slot[E], rows[E, max_rows]) of the twin over ``events`` = [(op, arg)]."""
    op = np.array([e[0] for e in events], dtype=np.uint32)
    arg = np.array([e[1] for e in events], dtype=np.uint32)
    depth = np.zeros(len(events), dtype=np.uint32)
    slot = np.zeros(len(events), dtype=np.uint32)
    rows = np.zeros((len(events), max_rows), dtype=np.uint32)
    rc = build_window_twin().twin_window_run(op.ctypes.data_as(_u32p), arg.ctypes.data_as(_u32p), len(events), max_rows,
                                             depth.ctypes.data_as(_u32p), slot.ctypes.data_as(_u32p), rows.ctypes.data_as(_u32p))
    return rc, depth, slot, rows


class RingModel:
    """The window as a list: the ids of the slices put since the last restart, oldest first, at most ``slices`` of them; and, per slot
    of the ring, the id of the slice that was written there last."""

    def __init__(self):
        self.slices, self.held, self.content = 0, [], {}

    def open(self, slices):
        self.slices, self.held, self.content = slices, [], {}

    def restart(self):
        self.held = []

    def put(self, slot, ident):
        assert 0 <= slot < self.slices
        self.content[slot] = ident
        self.held = (self.held + [ident])[-self.slices:]

    @property
    def depth(self):
        return max(len(self.held) - 1, 0)


def test_bindings_against_the_header():
    lib = load_library()
    bound = {s[0]: s for s in _abi.SYMBOLS}
    header = open(os.path.join(ROOT, "include", "cssm_pf.h")).read()
    for name in NAMES:
        assert name in bound and hasattr(lib, name), name
        m = re.search(r"^(?:int|uint32_t)\s+" + name + r"\(([^;]*)\);", header, re.M | re.S)
        assert m, name
        assert len([a for a in m.group(1).split(",") if a.strip()]) == len(bound[name][2]), name
    assert re.search(r"#define\s+CSSM_PF_NO_ROWS\s+0xffffffffu", header) and _abi.CSSM_PF_NO_ROWS == 0xFFFFFFFF
    assert bound["cssm_pf_window"][1] is C.c_int and bound["cssm_pf_window_depth"][1] is C.c_uint32
    assert len(bound["cssm_pf_step_interpolate"][2]) == 15 and bound["cssm_pf_step_interpolate"][2][4] is C.c_uint32
    assert bound["cssm_pf_step_interpolate"][2][8] == _u32p


def test_refusals_before_a_device_is_looked_at():
    lib = load_library()
    A = _abi.CSSM_EINVAL_ARG
    six = [None] * 6
    assert lib.cssm_pf_window(None, 4) == A and b"null handle" in lib.cssm_last_error()
    assert lib.cssm_pf_window(None, 0) == A
    assert lib.cssm_pf_window_depth(None) == 0
    nrows = C.c_uint32(7)
    assert lib.cssm_pf_step_interpolate(None, 1.0, 0.0, 1, 2, 0.975, None, None, C.byref(nrows), *six) == A
    assert b"null handle" in lib.cssm_last_error() and nrows.value == 7
    assert lib.cssm_pf_step_interpolate(None, 1.0, 0.0, 1, _abi.CSSM_PF_NO_ROWS, 0.975, None, None, None, *six) == A
    ms = np.full(2, 7.0)
    assert lib.cssm_pf_step_interpolate_last_ms(None, ms.ctypes.data_as(_dp)) == A and list(ms) == [7.0, 7.0]
    assert b"null argument" in lib.cssm_last_error()


@pytest.mark.parametrize("seed", range(6))
def test_window_twin_against_the_ring_model(seed):
    """Seeded sequences of open, put, restart and re-open: behind every event the twin's depth is the model's, a put goes to a slot of the
    ring, and row j sits in the slot whose last write was the (j + 1)-th newest slice -- never one overwritten since."""
    rng = np.random.default_rng(cases.SEED + seed)
    events = [(0, int(rng.integers(2, 7)))]
    for _ in range(400):
        u = rng.random()
        if u < 0.80:
            events.append((1, 0))
        elif u < 0.92:
            events.append((2, 0))
        else:
            events.append((0, int(rng.integers(2, 9))))
    max_rows = 9
    rc, depth, slot, rows = twin_run(events, max_rows)
    assert rc == 0
    model, ident = RingModel(), 0
    for e, (op, arg) in enumerate(events):
        if op == 0:
            model.open(arg)
        elif op == 2:
            model.restart()
        else:
            ident += 1
            model.put(int(slot[e]), ident)
        if op != 1:
            assert slot[e] == NONE
        assert depth[e] == model.depth, (e, events[e])
        assert depth[e] <= model.slices - 1
        for j in range(max_rows):
            if model.held and j <= model.depth:
                assert model.content[int(rows[e, j])] == model.held[-1 - j], (e, j)
            else:
                assert rows[e, j] == NONE, (e, j)
        if model.held:
            assert len(set(int(v) for v in rows[e, :model.depth + 1])) == model.depth + 1


def test_window_twin_edges():
    tw = build_window_twin()
    # a closed window takes no put; one slice is no window
    assert twin_run([(1, 0)], 2)[0] == 1
    assert twin_run([(0, 4), (0, 0), (1, 0)], 2)[0] == 3
    assert twin_run([(0, 1)], 2)[0] == 1
    assert twin_run([(0, 4), (7, 0)], 2)[0] == 2
    # opening and restarting leave depth 0 and no row; the first put is the base slice (depth 0, one row), the second a record
    rc, depth, slot, rows = twin_run([(0, 3), (2, 0), (1, 0), (1, 0), (1, 0), (1, 0), (2, 0), (1, 0), (0, 3), (1, 0)], 3)
    assert rc == 0 and list(depth) == [0, 0, 0, 1, 2, 2, 0, 0, 0, 0]
    assert list(rows[0]) == [NONE] * 3 and list(rows[2]) == [slot[2], NONE, NONE] and list(rows[5]) == [slot[5], slot[4], slot[3]]
    assert slot[5] == slot[2]                                   # the full ring overwrote its oldest slot
    assert list(rows[7]) == [slot[7], NONE, NONE]
    # rows of a call: min(lag, depth) + 1
    for slices, count, lag, want in ((4, 0, 0, 1), (4, 0, 3, 1), (4, 1, 3, 1), (4, 2, 0, 1), (4, 2, 3, 2), (4, 4, 3, 4), (4, 4, 2, 3), (16, 11, 10, 11),
                                     (16, 16, 10, 11)):
        assert tw.twin_window_rows(slices, count, lag) == want, (slices, count, lag)


def test_counted_budget_of_a_lineage_row():
    """A row is k_lineage_fill, the selection's enqueued passes and k_iv_finish: at most 8 launches, counted the way
    test_filter_intervals_host.test_counted_budget_of_a_row counts -- the compose and the fill share one launch, no iota."""
    for n in (1, 4097, 70001, 1 << 20):
        _, _, rounds, _ = twin_constants(n)
        assert 1 + rounds + 1 <= 8


# ---- the Python surface against a recording stub ---------------------------------------------------------------------------------------
D_STUB, N_STUB = 3, 11


class StubLib:
    """``NativePf.lib``: every call checks its argument count against ``_abi.SYMBOLS`` and records its inputs; cssm_pf_step_interpolate
    keeps a window as the library does (a base slice when it restarts) and fills row j of output q with 1000 (q + 1) + 10 j + component."""

    def __init__(self):
        self.calls, self.slices, self.count = [], 0, 0
        self.sig = {s[0]: s[2] for s in _abi.SYMBOLS}

    def cssm_pf_window(self, h, slices):
        assert len(self.sig["cssm_pf_window"]) == 2
        self.calls.append({"name": "cssm_pf_window", "slices": slices})
        self.slices, self.count = slices, 0
        return 0

    def cssm_pf_window_depth(self, h):
        return max(self.count - 1, 0)

    def cssm_pf_step_interpolate(self, *a):
        assert len(a) == len(self.sig["cssm_pf_step_interpolate"]) == 15
        h, t, y, has, lag, interval, ll, ess, nrows, *six = a
        self.calls.append({"name": "cssm_pf_step_interpolate", "t": t, "y": y, "has": has, "lag": lag, "interval": interval})
        self.count = min(self.count + (2 if self.count == 0 else 1), self.slices)
        ll._obj.value, ess._obj.value = -3.5, 9
        if lag == _abi.CSSM_PF_NO_ROWS:
            nrows._obj.value = 0
            return 0
        R = min(lag, self.count - 1) + 1
        nrows._obj.value = R
        for q, p in enumerate(six):
            w = D_STUB if q < 3 else 1
            out = np.ctypeslib.as_array(p, shape=((lag + 1) * w,)).reshape(lag + 1, w)
            out[:R] = 1000.0 * (q + 1) + 10.0 * np.arange(R)[:, None] + np.arange(w)[None, :]
        return 0

    def cssm_pf_step_interpolate_last_ms(self, h, ms):
        np.ctypeslib.as_array(ms, shape=(2,))[:] = (3.0, 2.0)
        return 0


def stub_pf() -> NativePf:
    pf = object.__new__(NativePf)
    pf.lib, pf._h, pf.n, pf.d, pf.generation = StubLib(), None, N_STUB, D_STUB, 0
    return pf


def test_native_pf_marshals_the_calls():
    pf = stub_pf()
    pf.window(4)
    assert pf.lib.calls[-1] == {"name": "cssm_pf_window", "slices": 4} and pf.window_depth() == 0
    ll, ess, nrows, rows = pf.step_interpolate(1.5, 2.0, lag=3, interval=0.9)
    c = pf.lib.calls[-1]
    assert (c["t"], c["y"], c["has"], c["lag"], c["interval"]) == (1.5, 2.0, 1, 3, 0.9) and pf.generation == 1
    assert (ll, ess, nrows) == (-3.5, 9, 2) and pf.window_depth() == 1
    m, lo, hi, em, el, eu = rows
    assert m.shape == lo.shape == hi.shape == (4, D_STUB) and em.shape == el.shape == eu.shape == (4,)
    for q, a in enumerate(rows):
        a2 = a.reshape(4, -1)
        np.testing.assert_array_equal(a2[:2], 1000.0 * (q + 1) + 10.0 * np.arange(2)[:, None] + np.arange(a2.shape[1])[None, :])
        assert np.isnan(a2[2:]).all()                       # rows the window does not reach were preset to NaN
    # a record without a datum; no rows
    ll, ess, nrows, rows = pf.step_interpolate(2.5, None)
    c = pf.lib.calls[-1]
    assert (c["y"], c["has"], c["lag"], c["interval"]) == (0.0, 0, _abi.CSSM_PF_NO_ROWS, 0.975) and nrows == 0 and pf.generation == 2
    assert rows[0].shape == (1, D_STUB) and np.isnan(rows[0]).all() and np.isnan(rows[3]).all()
    assert pf.step_interpolate(3.0, 1.0, has_obs=False, lag=0)[2] == 1 and pf.lib.calls[-1]["has"] == 0 and pf.lib.calls[-1]["y"] == 1.0
    assert pf.step_interpolate_last_ms() == (3.0, 2.0)
    for bad in (-1, 1 << 32):
        with pytest.raises(ValueError):
            pf.step_interpolate(4.0, 1.0, lag=bad)
    with pytest.raises(ValueError):
        pf.window(-1)
    assert pf.lib.calls[-1]["name"] == "cssm_pf_step_interpolate" and pf.lib.calls[-1]["t"] == 3.0   # refused before any call


def _expect(time, obs, j):
    return PfOut(time, obs, 4000.0 + 10.0 * j, CredibleInterval(5000.0 + 10.0 * j, 6000.0 + 10.0 * j), 1000.0 + 10.0 * j + np.arange(D_STUB),
                 [CredibleInterval(2000.0 + 10.0 * j + k, 3000.0 + 10.0 * j + k) for k in range(D_STUB)])


def _same_pfout(a: PfOut, b: PfOut):
    assert (a.time, a.observation, a.eta, a.etaIntervals, a.stateIntervals) == (b.time, b.observation, b.eta, b.etaIntervals, b.stateIntervals)
    np.testing.assert_array_equal(a.state, b.state)


def test_filter_interpolate_assembles_the_stream():
    flt = FilterInterpolate(cases.c2_model(), Resampling.systematicResampling)
    with pytest.raises(RuntimeError):
        flt.window(3)                                           # no handle yet
    flt._pf = stub_pf()
    flt._ensure = lambda n: flt._pf
    flt.window(3)
    st = flt._state(0.5, None, 0.0, N_STUB)
    data = [Data(1.0, 2.0), Data(2.0, None), Data(3.0, 4.0), Data(4.0, 1.0)]
    want_hist = [(0.5, None)]
    for i, dtm in enumerate(data):
        prev = st
        st, outs = flt.stepInterpolate(st, dtm, 2, interval=0.8)
        c = flt._pf.lib.calls[-1]
        assert (c["t"], c["y"], c["has"], c["lag"], c["interval"]) == (dtm.t, 0.0 if dtm.observation is None else dtm.observation,
                                                                       0 if dtm.observation is None else 1, 2, 0.8)
        assert (st.t, st.observation, st.ll, st.ess) == (dtm.t, dtm.observation, -3.5, 9) and st._generation == flt._pf.generation
        want_hist = (want_hist + [(dtm.t, dtm.observation)])[-3:]
        R = min(2, i + 1) + 1
        assert len(outs) == R
        for k, out in enumerate(outs):                          # oldest first: entry k is row R - 1 - k
            tt, ob = want_hist[len(want_hist) - R + k]
            _same_pfout(out, _expect(tt, ob, R - 1 - k))
        with pytest.raises(RuntimeError):
            flt.stepInterpolate(prev, dtm, 2)                   # not the current state any more
    # no rows: the state alone
    st, outs = flt.stepInterpolate(st, Data(5.0, 0.0), None)
    assert outs == [] and flt._pf.lib.calls[-1]["lag"] == _abi.CSSM_PF_NO_ROWS
    # a window that restarted (another call moved the cloud) takes the state before the datum as its base slice
    flt._pf.lib.count = 0
    st, outs = flt.stepInterpolate(st, Data(6.0, 3.0), 2)
    assert [(o.time, o.observation) for o in outs] == [(5.0, 0.0), (6.0, 3.0)]
    # a host Resample[A] has no ancestors on the device
    host = FilterInterpolate(cases.c2_model(), lambda samples, weights: samples)
    host._pf = stub_pf()
    with pytest.raises(RuntimeError):
        host.stepInterpolate(host._state(0.0, None, 0.0, N_STUB), Data(1.0, 1.0), 1)
