"""CPU-only checks of the single handle's backward-simulation smoother (include/cssm_pf.h: cssm_pf_smooth, cssm_pf_smooth_last_ms; an
EXTENSION -- the reference has no smoother beyond FilterInterpolate):

  * the bindings against the header, the refusals that need no handle, what the Python side hands over and what it refuses itself;
  * every kernel of cssm_smooth.hip is dispatched over the latent dimension, and one GPU test runs all sixteen;
  * the premise of the statistical GPU test (tests/test_gpu_smooth.py: test_truth): the sequential twin of the contract's backward
    simulation (tests/cpp/backsim_twin.c) on the ORACLE's history at N = 6000 is accepted by the exact smoother.  The device must equal
    the twin bit for bit, so what is established here on the CPU holds there.

The helpers of the premise are imported by tests/test_gpu_smooth.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import cases
from composablestatespacemodels_amd import Data, _abi, load_library
from composablestatespacemodels_amd.filter import FilterInterpolate, NativePf
from oracle import oracle
from test_fleet_smooth_host import kinds_of, oracle_history, pack_records, rank_truth, twin_traj

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A = _abi.CSSM_EINVAL_ARG
_dp, _u8p, _u32p = (C.POINTER(t) for t in (C.c_double, C.c_uint8, C.c_uint32))


# 1 ------------------------------------------------------------------------------------------------------------------------------
def test_the_calls_are_bound_exported_and_declared_as_bound():
    lib = load_library()
    sig = {s[0]: s for s in _abi.SYMBOLS}
    header = open(os.path.join(ROOT, "include", "cssm_pf.h")).read()
    ctype = {"cssm_pf*": C.c_void_p, "const uint8_t*": _u8p, "const double*": _dp, "double*": _dp, "uint32_t*": _u32p, "size_t": C.c_size_t,
             "double": C.c_double, "uint32_t": C.c_uint32, "int": C.c_int}
    for name in ("cssm_pf_smooth", "cssm_pf_smooth_last_ms"):
        assert name in sig and hasattr(lib, name)
        m = re.search(r"\bint " + name + r"\(([^)]*)\);", header)
        assert m, f"{name} is not declared in include/cssm_pf.h"
        args = [" ".join(a.split()[:-1]) for a in m.group(1).replace("\n", " ").split(",")]
        assert [ctype[a] for a in args] == list(sig[name][2]), (name, args)
        assert sig[name][1] is C.c_int
    assert _abi.CSSM_OPT_SMOOTH_TILE == int(re.search(r"#define CSSM_OPT_SMOOTH_TILE (\d+)", header).group(1)) == 15
    assert _abi.SMOOTH_TILE == int(re.search(r"#define CSSM_SMOOTH_TILE (\d+)", header).group(1))
    assert _abi.SMOOTH_TILE % 64 == 0 and 2 * _abi.MAX_DIM * _abi.SMOOTH_TILE * 8 <= 160 * 1024     # two blocks' tiles in a CU's LDS at d = 16
    # the section of the contract names both of its users, and its version did not move
    numerics = open(os.path.join(ROOT, "include", "cssm_numerics.h")).read()
    section = numerics[numerics.index("backward simulation (EXTENSION)"):]
    assert "cssm_fleet_smooth" in section and "cssm_pf_smooth" in section


def test_a_null_handle_is_refused_by_both_calls_and_the_array_is_left_alone():
    lib = load_library()
    t = np.arange(4.0); y = np.ones(4); ll = C.c_double(7.0)
    rc = lib.cssm_pf_smooth(None, t.ctypes.data_as(_dp), y.ctypes.data_as(_dp), None, 4, 10, 0.975, 0, C.byref(ll), *([None] * 6), None)
    assert rc == A and b"null" in lib.cssm_last_error() and ll.value == 7.0
    ms = np.full(3, 7.0)
    assert lib.cssm_pf_smooth_last_ms(None, ms.ctypes.data_as(_dp)) == A and list(ms) == [7.0, 7.0, 7.0]
    assert b"null" in lib.cssm_last_error()
    # the option is the single handle's: a null handle is refused before it is looked at, and a fleet has no such option
    assert lib.cssm_pf_set_option(None, _abi.CSSM_OPT_SMOOTH_TILE, 64) == A
    assert lib.cssm_fleet_set_option(None, _abi.CSSM_OPT_SMOOTH_TILE, 64) == A
    fleet_src = open(os.path.join(ROOT, "composablestatespacemodels_amd", "csrc", "cssm_fleet.hip")).read()
    assert "CSSM_OPT_SMOOTH_TILE" not in fleet_src


# 2 ------------------------------------------------------------------------------------------------------------------------------
class _Recorder:
    """stands where the library stands: keeps what cssm_pf_smooth was handed and fills the outputs with recognisable values"""

    def __init__(self, d):
        self.d, self.calls = d, []

    def cssm_pf_smooth(self, h, t, y, has, T, n_traj, interval, flags, ll, sm, slo, sup, em, elo, eup, traj):
        rows = T + 1
        self.calls.append({"t": np.ctypeslib.as_array(t, (T,)).copy(), "y": np.ctypeslib.as_array(y, (T,)).copy(),
                           "has": None if has is None else np.ctypeslib.as_array(has, (T,)).copy(), "T": T, "n_traj": n_traj,
                           "interval": interval, "flags": flags, "traj": traj is not None})
        ll._obj.value = -3.5
        np.ctypeslib.as_array(sm, (rows, self.d))[:] = np.arange(rows * self.d).reshape(rows, self.d)
        np.ctypeslib.as_array(elo, (rows,))[:] = np.arange(rows) + 0.25
        if traj is not None:
            np.ctypeslib.as_array(traj, (rows, n_traj))[:] = np.arange(rows * n_traj).reshape(rows, n_traj)
        return 0

    def cssm_pf_smooth_last_ms(self, h, ms):
        np.ctypeslib.as_array(ms, (3,))[:] = [1.0, 2.0, 3.0]
        return 0


def _handleless(n=10, d=2):
    pf = NativePf.__new__(NativePf)
    pf.n, pf.d, pf.generation, pf._h = n, d, 0, C.c_void_p()
    pf.lib = _Recorder(d)
    return pf


@pytest.mark.parametrize("want", [False, True])
def test_what_smooth_hands_over(want):
    pf = _handleless()
    out = pf.smooth([5.0, 6.0, 8.0], [2, 1, 4], [1, 0, 1], interval=0.9, want_trajectories=want)
    call = pf.lib.calls[0]
    assert list(call["t"]) == [5.0, 6.0, 8.0] and list(call["y"]) == [2.0, 1.0, 4.0] and list(call["has"]) == [1, 0, 1]
    assert (call["T"], call["n_traj"], call["interval"], call["flags"], call["traj"]) == (3, 10, 0.9, 0, want)   # None: min(N, 4096)
    assert len(out) == (8 if want else 7) and out[0] == -3.5 and pf.generation == 1
    assert out[1].shape == (4, 2) and out[4].shape == (4,)
    np.testing.assert_array_equal(out[1], np.arange(8).reshape(4, 2))
    np.testing.assert_array_equal(out[5], np.arange(4) + 0.25)
    if want:
        assert out[7].dtype == np.uint32 and out[7].shape == (4, 10)
        np.testing.assert_array_equal(out[7], np.arange(40).reshape(4, 10))
    pf.smooth([1.0], [0.0], n_traj=7)
    assert pf.lib.calls[1]["n_traj"] == 7 and pf.lib.calls[1]["interval"] == 0.975 and pf.lib.calls[1]["has"] is None
    big = _handleless(n=1 << 20)
    big.smooth([1.0], [0.0])
    assert big.lib.calls[0]["n_traj"] == _abi.FLEET_MAX_N
    assert pf.smooth_last_ms() == (1.0, 2.0, 3.0)


def test_what_smooth_refuses_before_any_library_call():
    pf = _handleless()
    for bad in (0, -1, _abi.FLEET_MAX_N + 1):
        with pytest.raises(ValueError, match="n_traj must be in"):
            pf.smooth([1.0], [0.0], n_traj=bad)
    for bad in (0.0, 1.5, -0.1, float("nan")):
        with pytest.raises(ValueError, match="interval must be in"):
            pf.smooth([1.0], [0.0], interval=bad)
    assert pf.lib.calls == [] and pf.generation == 0


def test_filter_interpolate_smooth_returns_what_interpolate_returns():
    data = [Data(3.0, 1.0), Data(4.0, None), Data(5.0, 4.0)]
    rng = np.random.default_rng(7)
    arrays = tuple(rng.normal(size=(4, 2)) for _ in range(3)) + tuple(rng.normal(size=4) for _ in range(3))
    seen = []

    class Pf:
        def smooth(self, t, y, has, n_traj, interval):
            seen.append(("smooth", list(t), list(has), n_traj, interval))
            return (-2.5,) + arrays

        def interpolate(self, t, y, has, interval, reference_pairing):
            return (-2.5,) + arrays

    fi = FilterInterpolate.__new__(FilterInterpolate)
    fi._ensure = lambda particles: Pf()
    ll, outs = fi.smooth(data, 300, n_traj=50, interval=0.9)
    ll2, outs2 = fi.interpolate(data, 300, 0.9)
    assert seen == [("smooth", [3.0, 4.0, 5.0], [1, 0, 1], 50, 0.9)] and ll == ll2 == -2.5 and len(outs) == len(outs2) == 4
    for a, b in zip(outs, outs2):
        assert type(a) is type(b) and (a.time, a.observation, a.eta, a.etaIntervals, a.stateIntervals) == (b.time, b.observation, b.eta, b.etaIntervals,
                                                                                                          b.stateIntervals)
        np.testing.assert_array_equal(a.state, b.state)
    assert [o.observation for o in outs] == [None, 1.0, None, 4.0]


# 3 ------------------------------------------------------------------------------------------------------------------------------
def test_every_kernel_is_instantiated_per_dimension_and_tested_over_all_sixteen():
    """The rule tests/test_fleet_smooth_host.py holds the fleet's smoother to: every kernel cssm_smooth.hip defines is launched through a
    function template that DISPATCH_D picks by the latent dimension, and one GPU test runs cases.dim_model(d) for d = 1 .. 16."""
    import importlib
    import inspect
    src = open(os.path.join(ROOT, "composablestatespacemodels_amd", "csrc", "cssm_smooth.hip")).read()
    defined = set(re.findall(r"__global__[^;{]*?void\s+(k_\w+)\(", src))
    assert defined == {"k_smooth_tiles", "k_smooth_fold", "k_smooth_rows"}
    launched = set(re.findall(r"hipLaunchKernelGGL\(\(?(k_\w+)<D", src))
    assert launched == defined and len(re.findall(r"DISPATCH_D\(", src)) == 4
    assert "atomic" not in src.split("#include", 1)[1].lower()     # no cross-block traffic inside a kernel: the launches order the passes
    mk = open(os.path.join(ROOT, "composablestatespacemodels_amd", "csrc", "Makefile")).read()
    assert "build/smooth.o" in re.search(r"^libcssm_pf\.so:(.*)$", mk, re.M).group(1)
    mod = importlib.import_module("test_gpu_smooth")
    fn = mod.test_every_latent_dimension
    marks = [m for m in fn.pytestmark if m.name == "parametrize" and m.args[0] == "d"]
    assert marks and list(marks[0].args[1]) == list(range(1, 17))
    body = inspect.getsource(fn)
    assert "cases.dim_model(d)" in body and ".smooth(" in body
    assert any(m.name == "gpu" for m in (mod.pytestmark if isinstance(mod.pytestmark, list) else [mod.pytestmark]))


# 4 ------------------------------------------------------------------------------------------------------------------------------
# The case of tests/test_gpu_smooth.py::test_truth: smoother_case("linear") (T = 12, the removed observations), a cloud beyond what a
# fleet holds, PREMISE_R replicates keyed PREMISE_SEED0 + r.  The truth is `rts` with the quantiles at the ranks' own probabilities.
PREMISE_N, PREMISE_M, PREMISE_R, PREMISE_SEED0 = 6000, 512, 16, 41000


def premise_case():
    import test_grid_smoother as tg
    return tg.smoother_case("linear")


def twin_rows(model, X, traj, t, interval=0.975):
    """(mean, lower, upper, eta_of_mean, eta_lower, eta_upper) per time index of the states X[s][:, traj[s]]: the oracle's summary, whose
    ranks are cssm_pf_summary's for as many values as there are trajectories."""
    o = oracle.OraclePf(model.descriptor(), traj.shape[1], 1)
    times = np.concatenate([[np.min(t)], t])
    rows = []
    for s in range(len(t) + 1):
        o.init(float(times[s]))
        o.set_particles(X[s][:, traj[s]])
        rows.append(o.summary(interval))
    return tuple(np.array([r[q] for r in rows]) for q in range(6))


def premise_twin(r):
    """(ll, traj, rows) of replicate r on the CPU: the oracle's forward pass, the twin's backward simulation, the oracle's summaries"""
    model, t, y, has = premise_case()
    seed = PREMISE_SEED0 + r
    ll, X, Anc = oracle_history(model, PREMISE_N, seed, (t, y, has))
    traj = twin_traj(X, Anc, pack_records(model, PREMISE_N, seed, t, y, has), kinds_of(model), seed, PREMISE_M)
    return ll, traj, twin_rows(model, X, traj, t)


def test_the_premise_the_twin_at_six_thousand_particles_is_accepted_by_the_exact_smoother():
    """z = (replicate mean - truth) / sqrt(s^2 / R) over the 13 rows, rms and max (criteria: rms <= 3, max <= 8), under the first
    PREMISE_SEED0 written down (41000), R = 16, N = 6000, n_traj = 512, measured on the CPU twin:
        mean 0.97 / 1.43   lower 0.86 / 1.41   upper 0.74 / 1.45   eta_lower 0.87 / 2.21   eta_upper 0.76 / 1.40   -- accepted"""
    import test_grid_smoother as tg
    model, t, y, has = premise_case()
    tr = rank_truth(model, t, y, has, PREMISE_M)
    outs = [(ll,) + rows for ll, _, rows in (premise_twin(r) for r in range(PREMISE_R))]
    runs = tg.stack(outs)
    assert runs[0].shape == (PREMISE_R, len(t) + 1, 1)
    print(f"\nlinear, T = {len(t)}, N = {PREMISE_N}, n_traj = {PREMISE_M}, R = {PREMISE_R}")
    tg.check_smoothing("twin", runs, tr)
