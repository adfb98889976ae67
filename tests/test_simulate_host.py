"""CPU-only checks of SimulateData's host side (include/cssm_pf.h: cssm_simulate, cssm_simulate_from, cssm_fleet_simulate): the ctypes
view against the header, every refusal that is decided before the first device call returned without a device, and the pure Python of
composablestatespacemodels_amd/simulate.py and formats.py -- the row splitting, to_data(), the CSV / JSON lines and their round trips,
and the step bookkeeping of the lazy iterators (a recording stub stands in for the native call)."""
from __future__ import annotations

import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import cases
from composablestatespacemodels_amd import _abi, formats as F
from composablestatespacemodels_amd.filter import NativePfFleet
from composablestatespacemodels_amd.model import Model, Parameters, Sde, SdeParameter, TimedObservation
from composablestatespacemodels_amd.simulate import SimulateData, SimulatedPoint, points_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEY = 0x51DA7A
_dp = C.POINTER(C.c_double)
_OU = SdeParameter.ouParameter(0.0, 1.0, 0.2, 0.0, 0.3)


def test_the_header_declares_what_the_ctypes_view_binds():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cssm_pf.h")).read(), flags=re.S)
    bound = {n: (res, args) for n, res, args in _abi.SYMBOLS}
    for name, nargs in (("cssm_simulate", 9), ("cssm_simulate_from", 11), ("cssm_simulate_last_ms", 1), ("cssm_fleet_simulate", 8),
                        ("cssm_fleet_simulate_last_ms", 2)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", src)
        assert m and len(m.group(1).split(",")) == nargs == len(bound[name][1]), name
        assert hasattr(_abi.load_library(), name)
    draws = open(os.path.join(ROOT, "include", "cssm_obs_draws.h")).read()
    assert re.search(r"#define CSSM_SIM_STEP_ROW0 0xFFFFFFFFu", draws) and _abi.CSSM_SIM_STEP_ROW0 == 0xFFFFFFFF


def _raw(model, n, t0, times, out, device=0):
    lib = _abi.load_library()
    desc = model if hasattr(model, "ptr") else model.descriptor()
    t = None if times is None else np.ascontiguousarray(times, dtype=np.float64)
    rc = lib.cssm_simulate(desc.ptr(), n, KEY, float(t0), None if t is None else t.ctypes.data_as(_dp), 0 if t is None else len(t), 0, device,
                           None if out is None else out.ctypes.data_as(_dp))
    return rc, _abi.last_error()


def without_scale(model):
    """the model's descriptor with the leftmost leaf's scale taken away (the Python constructors refuse such a model themselves)"""
    desc = model.descriptor()
    desc.leaf_array[0].has_scale = 0
    return desc


def refusals(out):
    c2 = cases.c2_model()
    noscale = without_scale(Model.linear(Sde.ouProcess(1)).run(Parameters.apply(0.1, _OU)))
    negbin = without_scale(Model.negativeBinomial(Sde.ouProcess(1)).run(Parameters.apply(0.1, _OU)))
    t_df0 = Model.studentsT(Sde.ouProcess(1), 0).run(Parameters.apply(0.1, _OU))
    lgcp = Model.lgcp(Sde.ouProcess(1)).run(Parameters.apply(None, _OU))
    ts = [1.0, 2.0, 3.0]
    return (((c2, 2, 0.0, ts, None), "null argument"),
            ((c2, 2, 0.0, None, out), None),                       # (T = 0 needs no times: not a refusal -- it reaches the device)
            ((c2, 0, 0.0, ts, out), "n_paths"),
            ((c2, 2**32, 0.0, ts, out), "n_paths"),
            ((c2, 2, 0.0, [1.0, float("nan"), 3.0], out), "t[1] is not finite"),
            ((c2, 2, float("inf"), ts, out), "t0 is not finite"),
            ((c2, 2, 2.0, ts, out), "is before t0"),
            ((c2, 2, 0.0, [1.0, 3.0, 2.0], out), "non-decreasing"),
            ((lgcp, 2, 0.0, ts, out), "log-Gaussian Cox"),
            ((noscale, 2, 0.0, ts, out), "Must provide SD parameter"),
            ((negbin, 2, 0.0, ts, out), "No scale parameter provided to Negativebinomial"),
            ((t_df0, 2, 0.0, ts, out), "df >= 1"))


def test_refusals_come_before_any_device_call():
    """Device 10 000 does not exist anywhere: a refusal that names its own cause was made before the device was looked at."""
    out = np.full((4, 6, 2), -7.0)
    for args, word in refusals(out):
        rc, msg = _raw(*args, device=10000)
        if word is None:
            assert rc in (_abi.CSSM_EHIP, _abi.CSSM_EINVAL_ARG) and ("device" in msg or "HIP" in msg), msg
        else:
            assert rc == _abi.CSSM_EINVAL_ARG and word in msg, (word, rc, msg)
        assert np.all(out == -7.0), word
    lib = _abi.load_library()
    t = np.array([1.0]); x = np.zeros((3, 2))
    d = cases.c2_model().descriptor()
    call = lambda xx, first, tt: lib.cssm_simulate_from(d.ptr(), 2, KEY, None if xx is None else xx.ctypes.data_as(_dp), first, 0.0, tt.ctypes.data_as(_dp),
                                                        len(tt), 0, 10000, out.ctypes.data_as(_dp))
    assert call(None, 0, t) == _abi.CSSM_EINVAL_ARG and "null argument" in _abi.last_error()
    assert call(x, 0xFFFFFFFF, t) == _abi.CSSM_EINVAL_ARG and "first_step + T" in _abi.last_error()
    bad = x.copy(); bad[1, 1] = np.inf
    assert call(bad, 0, t) == _abi.CSSM_EINVAL_ARG and "component 1 of path 1" in _abi.last_error()
    assert call(x, 0, np.array([-1.0])) == _abi.CSSM_EINVAL_ARG and "is before t0" in _abi.last_error()
    assert np.all(out == -7.0)
    ms = C.c_double()
    assert lib.cssm_simulate_last_ms(None) == _abi.CSSM_EINVAL_ARG
    # the fleet's call-level refusals need no fleet
    off = np.array([0, 1], dtype=np.uint64); rc = np.zeros(1, dtype=np.int32); ky = np.zeros(1, dtype=np.uint64); t0 = np.zeros(1)
    u64, ip = C.POINTER(C.c_uint64), C.POINTER(C.c_int)
    assert lib.cssm_fleet_simulate(None, 1, t0.ctypes.data_as(_dp), off.ctypes.data_as(u64), t.ctypes.data_as(_dp), ky.ctypes.data_as(u64),
                                   out.ctypes.data_as(_dp), rc.ctypes.data_as(ip)) == _abi.CSSM_EINVAL_ARG
    assert "null argument" in _abi.last_error()
    assert lib.cssm_fleet_simulate_last_ms(None, C.byref(ms)) == _abi.CSSM_EINVAL_ARG


def _rows(T1, d, n, base=0.0):
    return base + np.arange(T1 * (d + 3) * n, dtype=np.float64).reshape(T1, d + 3, n)


def test_row_splitting_and_to_data():
    rows = _rows(3, 2, 4)
    pts = points_of(0.5, [1.0, 2.5], rows, path=1)
    assert [p.t for p in pts] == [0.5, 1.0, 2.5]
    for h, p in enumerate(pts):
        assert np.array_equal(p.sdeState, rows[h, :2, 1]) and (p.gamma, p.eta, p.observation) == tuple(rows[h, 2:, 1])
        assert p.to_data() == TimedObservation(p.t, p.observation)
    tail = points_of(None, [1.0, 2.5, 4.0], rows)
    assert [p.t for p in tail] == [1.0, 2.5, 4.0] and tail[0].observation == rows[0, 4, 0]
    with pytest.raises(ValueError, match="rows for"):
        points_of(0.5, [1.0], rows)
    p = pts[0]
    p.sdeState[0] = -1.0
    assert rows[0, 0, 1] != -1.0      # a point owns its state
    # the fleet's split: series k owns the rows off[k] + k .. off[k + 1] + k
    off = np.array([0, 0, 1, 6, 9], dtype=np.uint64)
    per = NativePfFleet._split(off, _rows(13, 1, 1), 1)
    assert [len(v) for v in per] == [1, 2, 6, 4] and per[2][0, 0, 0] == _rows(13, 1, 1)[3, 0, 0]


def test_csv_and_json_lines_round_trip(tmp_path):
    p = SimulatedPoint(0.1, 3.0, 2.718281828459045, 1.0, np.array([1.0, -0.25, 1e-300]))
    line = F.simulated_csv(p)
    assert line == "0.1, 3.0, 2.718281828459045, 1.0, 1.0, -0.25, 1e-300"      # Show[Data]: t, y, eta, gamma, state
    q = F.simulated_from_csv(line)
    assert (q.t, q.observation, q.eta, q.gamma) == (p.t, p.observation, p.eta, p.gamma) and np.array_equal(q.sdeState, p.sdeState)
    missing = SimulatedPoint(0.2, None, 0.5, -0.7, np.array([0.3]))
    assert F.simulated_csv(missing).startswith("0.2, NA, 0.5, -0.7, ") and F.simulated_from_csv(F.simulated_csv(missing)).observation is None
    js = F.simulated_to_json(p, [1, 2])
    o = json.loads(js)
    assert list(o) == ["t", "observation", "eta", "gamma", "sdeState"] and o["sdeState"] == [{"value": [1.0]}, {"value": [-0.25, 1e-300]}]
    q = F.simulated_from_json(js)
    assert (q.t, q.observation, q.eta, q.gamma) == (p.t, p.observation, p.eta, p.gamma) and np.array_equal(q.sdeState, p.sdeState)
    assert "observation" not in json.loads(F.simulated_to_json(missing, [1])) and F.simulated_from_json(F.simulated_to_json(missing, [1])).observation is None
    # a simulated series feeds the observation writers and comes back through the existing readers
    pts = [p, missing]
    F.write_csv_observations(str(tmp_path / "a.csv"), [v.to_data() for v in pts])
    assert F.read_csv_observations(str(tmp_path / "a.csv")) == [TimedObservation(0.1, 3.0), TimedObservation(0.2, None)]
    F.write_csv_simulated(str(tmp_path / "b.csv"), pts)
    assert F.read_csv_observations(str(tmp_path / "b.csv")) == [TimedObservation(0.1, 3.0), TimedObservation(0.2, None)]   # (t, y lead the line)
    F.write_json_simulated(str(tmp_path / "b.json"), pts, [3])
    back = [F.simulated_from_json(l) for l in open(tmp_path / "b.json")]
    assert np.array_equal(back[0].sdeState, p.sdeState) and back[1].observation is None
    assert F.read_json_observations(str(tmp_path / "b.json")) == [TimedObservation(0.1, 3.0), TimedObservation(0.2, None)]


class _Stub(SimulateData):
    """SimulateData whose native seam records what it is asked for and returns rows that name their own time index."""

    def __init__(self):
        super().__init__(cases.c2_model(), seed=11)
        self._key = 0xABCDEF
        self.calls = []
        self.count = 0

    def _call(self, key, first_step, t0, x, times):
        self.calls.append((key, first_step, t0, None if x is None else np.array(x), list(times)))
        rows = len(times) + (1 if first_step is None else 0)
        out = np.zeros((rows, 6, 1))
        for r in range(rows):
            out[r, :, 0] = self.count
            self.count += 1
        return out


def test_the_lazy_iterators_count_their_steps_on():
    s = _Stub()
    it = s.simMarkov(0.25, block=4)
    pts = [next(it) for _ in range(13)]
    assert [p.observation for p in pts] == [float(i) for i in range(13)]                 # every time index once, in order
    t, want = 0.0, [0.0]
    for _ in range(12):
        t = t + 0.25
        want.append(t)
    assert [p.t for p in pts] == want
    # block 0: time indices 0 .. 3 from the initial draw (steps row0, 0, 1, 2); block 1 continues at step 3 from the state of index 3,
    # block 2 at step 7 from index 7, block 3 at step 11 from index 11
    assert [(c[0], c[1], c[2]) for c in s.calls] == [(0xABCDEF, None, 0.0), (0xABCDEF, 3, 0.75), (0xABCDEF, 7, 1.75), (0xABCDEF, 11, 2.75)]
    assert [len(c[4]) for c in s.calls] == [3, 4, 4, 4] and s.calls[1][4] == [1.0, 1.25, 1.5, 1.75]
    assert s.calls[0][3] is None and np.array_equal(s.calls[1][3], np.full(3, 3.0)) and np.array_equal(s.calls[2][3], np.full(3, 7.0))
    # a lazy iterator asks for nothing before it is read
    n = len(s.calls)
    it2 = s.simRegular(0.1)
    assert len(s.calls) == n
    next(it2)
    assert len(s.calls) == n + 1 and len(s.calls[-1][4]) == SimulateData.BLOCK - 1
    obs = s.observations
    first = next(obs)
    assert first.t == 0.0 and abs(s.calls[-1][4][0] - 0.1) < 1e-15
    with pytest.raises(ValueError, match="at least two"):
        s.simMarkov(0.1, block=1)


def test_sim_pomp_model_and_sim_step_ask_for_what_they_say():
    s = _Stub()
    pts = s.simPompModel(2.0)(iter([2.5, 2.5, 4.0]))
    assert s.calls[-1][:3] == (0xABCDEF, None, 2.0) and s.calls[-1][4] == [2.5, 2.5, 4.0] and [p.t for p in pts] == [2.0, 2.5, 2.5, 4.0]
    step = s.simStep(0.5)
    a = step(pts[-1])
    b = step(a)
    c = step(b, step=40)
    assert [(k[1], k[2], k[4]) for k in s.calls[-3:]] == [(0, 4.0, [4.5]), (1, 4.5, [5.0]), (40, 5.0, [5.5])]
    assert (a.t, b.t, c.t) == (4.5, 5.0, 5.5) and np.array_equal(s.calls[-1][3], b.sdeState)


def test_the_host_plan_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """csrc/cssm_simulate_plan.cpp (every refusal, the records) over csrc/cssm_model.cpp as a stand-alone program with its own main
    (tests/cpp/simulate_plan_main.cpp), built with -fsanitize=address,undefined and run here: host code, no device, nothing preloaded."""
    import subprocess
    csrc = os.path.join(ROOT, "composablestatespacemodels_amd", "csrc")
    exe = str(tmp_path / "simulate_plan_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-mfma", "-Wall", "-Werror", "-fno-omit-frame-pointer",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + csrc, "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "simulate_plan_main.cpp"), os.path.join(csrc, "cssm_simulate_plan.cpp"),
                           os.path.join(csrc, "cssm_model.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "simulate_plan: ok" in r.stdout, r.stdout + r.stderr
