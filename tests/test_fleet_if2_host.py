"""CPU-only checks of iterated filtering on a fleet (include/cssm_pf.h: cssm_fleet_if2, an EXTENSION -- the reference has no likelihood
maximiser; IF2 of Ionides, Nguyen, Atchade, Stoev and King 2015):

  * the bindings against the header and every refusal that is made before the fleet is looked at;
  * the sequential twin of the contract's section (tests/cpp/if2_twin.c, written from include/cssm_numerics.h alone): with a frozen swarm
    (every rw_sd = 0) one iteration IS the oracle's ll_filter under the iteration's key, bit for bit -- ll, ESS, cloud, ancestors -- which
    ties the twin to the oracle; a slot with sd 0 never changes a bit, freeing another slot does not change the draws of the first, two
    runs under one seed are equal;
  * the statistical acceptance of the method on the twin (below).

Acceptance.  ``cases.linear_model()`` (Brownian latent, Gaussian observation: Kalman-tractable) on ``cases.gaussian_series(ACC_T)``; free
are the observation log-scale (slot 0) and the latent log-variance rate (slot 3), p = 2; m0 and log c0 stay fixed (rw_sd 0).  l_max is
the maximum of the exact Kalman log-likelihood (``grid_reference.kalman``, the likelihood tests/test_smc2_host.py builds on) found by
``scipy.optimize.minimize`` (Nelder-Mead) from several starts.  Criterion, for every search: 2 (l_max - l_Kalman(theta_hat)) <= 5.99, the
95 % point of chi-square with 2 degrees of freedom -- theta_hat, the final swarm mean, lies inside the 95 % likelihood-ratio region.  The
same criterion must REJECT every starting point, and the final mean of a run with every has_obs = 0, where the swarm only random-walks.

Measured on the twin with the settings below (the test prints the figures on every run; none of the seeds was retried or dropped):
l_max = -70.525115 at (log obs sd, log sigma) = (-0.8832, -1.1651); 2 dl of the four searches 1.002, 0.001, 0.239, 0.005 (accepted, the
largest a sixth of 5.99); of their starting points 78.15, 17.10, 57.22, 173.29 (rejected); of the final means with every has_obs = 0
76.36, 19.18, 43.67, 157.73 (rejected).  4 searches x N = 300 x M = 40 iterations x T = 60 records take 2 s on one core.

The helpers that build the twin and run a search through it are imported by tests/test_gpu_fleet_if2.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import cases
import grid_reference as gr
from composablestatespacemodels_amd import _abi, load_library
from composablestatespacemodels_amd.filter import NativePfFleet
from oracle import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A, D_ = _abi.CSSM_EINVAL_ARG, _abi.CSSM_EINVAL_DESC
_dp, _u8p, _u32p, _u64p, _i32p = (C.POINTER(t) for t in (C.c_double, C.c_uint8, C.c_uint32, C.c_uint64, C.c_int32))
_TWIN = None
U64 = 2**64 - 1


def build_if2_twin(out_dir=None) -> C.CDLL:
    """tests/cpp/if2_twin.c built with the gcc line of the other twins (once per process)."""
    global _TWIN
    if _TWIN is None:
        import tempfile
        so = os.path.join(str(out_dir or tempfile.mkdtemp(prefix="if2_twin_")), "if2_twin.so")
        subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-mfma", "-std=c99", "-shared", "-fPIC", "-o", so,
                               os.path.join(ROOT, "tests", "cpp", "if2_twin.c"), "-lm"])
        lib = C.CDLL(so)
        lib.twin_if2.argtypes = [_i32p, C.c_uint32, _dp, _dp, _dp, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint32, _dp, _dp, _u8p, _dp, _dp, _dp,
                                 _i32p, _dp, _u32p, _u32p]
        lib.twin_if2.restype = C.c_int
        lib.twin_if2_normal.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32]
        lib.twin_if2_normal.restype = C.c_double
        _TWIN = lib
    return _TWIN


def layout_of(model) -> np.ndarray:
    """cssm_fleet_if2_layout's integers for a model."""
    lib = load_library()
    cnt = C.c_size_t()
    _abi.check(lib.cssm_fleet_if2_layout(model.descriptor().ptr(), None, 0, C.byref(cnt)))
    out = np.zeros(cnt.value, dtype=np.int32)
    _abi.check(lib.cssm_fleet_if2_layout(model.descriptor().ptr(), out.ctypes.data_as(_i32p), out.size, C.byref(cnt)))
    return out


def cooling(c, first, iters) -> np.ndarray:
    out = np.zeros(iters)
    _abi.check(load_library().cssm_fleet_if2_cooling(float(c), int(first), int(iters), out.ctypes.data_as(_dp)))
    return out


def theta_of(model) -> np.ndarray:
    return np.array(model.parameters().flattenParams(), dtype=np.float64)


def twin_search(model, n, data, rw_sd, cool_c, iters, seed, theta0=None, swarm0=None, first_iter=0):
    """One search of the twin: a dict with the keys of ``NativePfFleet.if2(..., want_swarm=True, want_last=True)`` for one series."""
    t, y, has = (np.ascontiguousarray(a, dtype=ty) for a, ty in zip(data, (np.float64, np.float64, np.uint8)))
    lay = layout_of(model)
    d, nt = int(lay[0]), int(lay[1])
    T = len(t)
    out = {"theta_mean": np.full((iters, nt), np.nan), "ll": np.full(iters, np.nan), "rc": 0, "ll_t": np.full(T, np.nan),
           "ess_t": np.full(T, -1, dtype=np.int32), "x": np.full((d, n), np.nan), "anc": np.full(n, 0xffffffff, dtype=np.uint32)}
    swarm = (np.repeat(np.asarray(theta0, dtype=np.float64).reshape(nt, 1), n, axis=1) if swarm0 is None
             else np.array(swarm0, dtype=np.float64).reshape(nt, n))
    swarm = np.ascontiguousarray(swarm)
    out["swarm"] = swarm
    if T == 0:
        return out
    sd = np.ascontiguousarray(rw_sd, dtype=np.float64)
    cool = cooling(cool_c, first_iter, iters)
    ll_t, ess_t, x, anc = np.zeros(T), np.zeros(T, dtype=np.int32), np.zeros((d, n)), np.zeros(n, dtype=np.uint32)
    fail = C.c_uint32(0)
    rc = build_if2_twin().twin_if2(lay.ctypes.data_as(_i32p), n, swarm.ctypes.data_as(_dp), sd.ctypes.data_as(_dp), cool.ctypes.data_as(_dp),
                                   first_iter, iters, int(seed) & U64, T, t.ctypes.data_as(_dp), y.ctypes.data_as(_dp), has.ctypes.data_as(_u8p),
                                   out["theta_mean"].ctypes.data_as(_dp), out["ll"].ctypes.data_as(_dp), ll_t.ctypes.data_as(_dp),
                                   ess_t.ctypes.data_as(_i32p), x.ctypes.data_as(_dp), anc.ctypes.data_as(_u32p), C.byref(fail))
    assert rc in (0, _abi.CSSM_ENONFINITE), rc
    out["rc"] = rc
    if rc == 0:
        out.update(ll_t=ll_t, ess_t=ess_t, x=x, anc=anc)
    return out


# 1 ------------------------------------------------------------------------------------------------------------------------------
def test_the_contract_names_the_stream_and_the_twin_states_the_normal():
    src = open(os.path.join(ROOT, "include", "cssm_numerics.h")).read()
    assert re.search(r"#define CSSM_STREAM_IF2 \(12u\)", src) and _abi.CSSM_STREAM_IF2 == 12
    assert "iterated filtering (EXTENSION)" in src
    tags = re.findall(r"#define CSSM_STREAM_\w+ \(?(\d+)u\)?", src + open(os.path.join(ROOT, "include", "cssm_obs_draws.h")).read())
    assert sorted(int(v) for v in tags) == list(range(13))      # no other stream of the contract has the tag
    tw = build_if2_twin()
    key = 0x0123456789abcdef
    for i, when, j in ((0, 0, 0), (5, 3, 1), (4095, 12, 2), (7, 1, 3), (7, 1, 80)):
        # normal j of the stream (key, particle i, perturbation `when`, tag 12): element j & 1 of pair j >> 1
        assert tw.twin_if2_normal(key, i, when, j) == oracle.c_normals(key, i, when, 12, j >> 1, 1)[0][j & 1]
    cool = cooling(0.5, 0, 101)
    assert cool[0] == 1.0 and cool[50] == 0.5 and abs(cool[100] - 0.25) < 1e-15 and np.all(np.diff(cool) < 0)
    np.testing.assert_array_equal(cooling(0.5, 30, 10), cool[30:40])


# 2 ------------------------------------------------------------------------------------------------------------------------------
def test_the_calls_are_bound_exported_and_declared_as_bound():
    lib = load_library()
    sig = {s[0]: s for s in _abi.SYMBOLS}
    header = open(os.path.join(ROOT, "include", "cssm_pf.h")).read()
    ctype = {"cssm_fleet*": C.c_void_p, "const cssm_model_desc*": _abi._descp, "const uint8_t*": _u8p, "const double*": _dp, "double*": _dp,
             "const uint64_t*": _u64p, "uint32_t*": _u32p, "int32_t*": _i32p, "int*": C.POINTER(C.c_int), "double": C.c_double,
             "uint32_t": C.c_uint32, "size_t": C.c_size_t, "size_t*": C.POINTER(C.c_size_t)}
    for name in ("cssm_fleet_if2", "cssm_fleet_if2_last_ms", "cssm_fleet_if2_cooling", "cssm_fleet_if2_layout"):
        assert name in sig and hasattr(lib, name)
        m = re.search(r"\bint " + name + r"\(([^)]*)\);", header)
        assert m, f"{name} is not declared in include/cssm_pf.h"
        args = [" ".join(a.split()[:-1]) for a in m.group(1).replace("\n", " ").split(",")]
        assert [ctype[a] for a in args] == list(sig[name][2]), (name, args)
        assert sig[name][1] is C.c_int
    assert _abi.IF2_MAX_THETA == 81


def _call(lib, desc=None, null=(), off=(0, 2), n_theta=4, rw_sd=(0.1, 0.0, 0.0, 0.1), cool=0.5, first=0, iters=2, swarm=False):
    desc = cases.linear_model().descriptor() if desc is None else desc
    off = np.asarray(off, dtype=np.uint64)
    arr = {"theta0": np.zeros(max(n_theta, 1)), "rw_sd": np.asarray(rw_sd, dtype=np.float64), "seeds": np.zeros(1, dtype=np.uint64), "off": off,
           "t": np.arange(4.0), "y": np.ones(4), "mean": np.zeros(max(iters, 1) * max(n_theta, 1)), "ll": np.zeros(max(iters, 1)),
           "rc": np.zeros(1, dtype=np.int32), "swarm0": np.zeros(max(n_theta, 1) * 4)}
    p = lambda name, ty: None if name in null else arr[name].ctypes.data_as(ty)
    return lib.cssm_fleet_if2(None, None if "desc" in null else desc.ptr(), p("theta0", _dp), p("swarm0", _dp) if swarm else None, n_theta,
                              p("rw_sd", _dp), cool, first, iters, 0, p("seeds", _u64p), p("off", _u64p), p("t", _dp), p("y", _dp), None,
                              p("mean", _dp), p("ll", _dp), None, None, None, None, None, p("rc", C.POINTER(C.c_int)))


def test_whole_call_refusals_are_made_before_the_fleet_is_looked_at():
    lib = load_library()
    err = lambda: lib.cssm_last_error()
    for name in ("desc", "rw_sd", "seeds", "off"):
        assert _call(lib, null=(name,)) == A and b"null argument" in err(), name
    assert _call(lib, null=("theta0",)) == A and b"theta0 and swarm0 are both null" in err()
    assert _call(lib, null=("theta0",), swarm=True) == A and b"null fleet" in err()          # a swarm alone is a start
    for name in ("mean", "ll", "rc"):
        assert _call(lib, null=(name,)) == A and b"null output" in err(), name
    assert _call(lib, off=(1, 2)) == A and b"off[0] must be 0" in err()
    for name in ("t", "y"):
        assert _call(lib, null=(name,)) == A and b"null data" in err(), name
    for bad in (-0.1, np.nan, np.inf, -np.inf):
        assert _call(lib, rw_sd=(0.1, 0.0, bad, 0.1)) == A and b"rw_sd[2]" in err() and b"finite and not negative" in err(), bad
    for bad in (0, 1000001):
        assert _call(lib, iters=bad) == A and b"n_iters must be in [1, 1000000]" in err(), bad
    assert _call(lib, first=2**31 - 1, iters=2) == A and b"first_iter + n_iters" in err()
    for bad in (0.0, -0.5, 1.0000001, np.nan, np.inf):
        assert _call(lib, cool=bad) == A and b"cooling_fraction_50" in err() and b"(0, 1]" in err(), bad
    assert _call(lib, desc=cases.c4_model().descriptor(), n_theta=5, rw_sd=(0.0,) * 5) == D_ and b"LGCP" in err() and b"not served" in err()
    for bad in (3, 5):
        assert _call(lib, n_theta=bad, rw_sd=(0.0,) * bad) == A and b"the descriptor flattens to 4" in err(), bad
    # every earlier refusal wins over the later ones; the last one made without a fleet is the fleet's absence
    assert _call(lib, off=(1, 2), cool=7.0, iters=0) == A and b"off[0] must be 0" in err()
    assert _call(lib) == A and b"null fleet" in err()
    assert _call(lib, cool=1.0) == A and b"null fleet" in err()                              # 1 is allowed: no cooling
    ms = np.full(1, 7.0)
    assert lib.cssm_fleet_if2_last_ms(None, ms.ctypes.data_as(_dp)) == A and ms[0] == 7.0


def test_the_layout_of_known_models():
    lay = layout_of(cases.linear_model())                      # [log obs sd, m0, log c0, log sigma]
    assert list(lay[:5]) == [1, 4, 1, 0, 0]                   # d, n_theta, CSSM_OBS_GAUSSIAN, no df, the scale in slot 0
    assert list(lay[5:15]) == [0, 0, 0, 0, lay[9], 1, 2, -1, -1, 3] and list(lay[15:]) == [0, 1, 1, 0]
    lay = layout_of(cases.c2_model())                          # ou(1): m0 c0 phi mu sigma | seasonal ou(2): the same, scalars repeated
    d, nt = int(lay[0]), int(lay[1])
    assert (d, nt, int(lay[4])) == (3, 10, -1)
    comps = lay[5:5 + 10 * d].reshape(d, 10)
    assert comps[:, 0].tolist() == [2, 2, 2] and comps[:, 1].tolist() == [0, 1, 1] and comps[:, 2].tolist() == [0, 0, 1]
    assert comps[0, 5:].tolist() == [0, 1, 3, 2, 4] and comps[1, 5:].tolist() == [5, 6, 8, 7, 9] and comps[2, 5:].tolist() == [5, 6, 8, 7, 9]
    assert lay[5 + 10 * d:].tolist() == [1, 1, 0, 0, 0, 1, 1, 0, 0, 0]
    lay = layout_of(cases.gen_brownian_seasonal_gaussian())    # scale | gen-brownian m0 c0 mu sigma | ou(2) with two-entry m0 and mu
    assert int(lay[4]) == 0 and int(lay[1]) == 5 + 7
    comps = lay[5:35].reshape(3, 10)
    assert comps[0, 5:].tolist() == [1, 2, 3, -1, 4] and comps[1, 5:].tolist() == [5, 7, 9, 8, 11] and comps[2, 5:].tolist() == [6, 7, 10, 8, 11]


# 3 ------------------------------------------------------------------------------------------------------------------------------
FROZEN = ["c1", "c2", "c3", "linear", "negbin", "zip", "bernoulli", "studentt", "beta", "gbsg", "euler"]   # every non-LGCP kind, every SDE


def ragged(name, T=9):
    """A series with an unobserved record and a repeated time (dt = 0)."""
    model, t, y, has = cases.literal_case(name, T)
    t = t.copy(); has = has.copy()
    t[4] = t[3]
    has[2] = 0
    return model, (t, y, has)


@pytest.mark.parametrize("name", FROZEN)
def test_a_frozen_swarm_is_the_oracles_filter_under_the_iteration_key(name):
    model, data = ragged(name)
    n, seed = 37, cases.SEED + 3
    th = theta_of(model)
    got = twin_search(model, n, data, np.zeros(len(th)), 0.5, 1, seed, theta0=th)
    o = oracle.OraclePf(model.descriptor(), n, int(load_library().cssm_pf_run_key(seed, 1)))
    ll, ll_t, ess_t, _ = o.filter(*data)
    assert got["rc"] == 0 and got["ll"][0] == ll
    np.testing.assert_array_equal(got["ll_t"], ll_t); np.testing.assert_array_equal(got["ess_t"], ess_t)
    np.testing.assert_array_equal(got["x"], o.proposed()); np.testing.assert_array_equal(got["anc"], o.ancestors())
    np.testing.assert_array_equal(got["x"][:, got["anc"]], o.particles())
    # nothing moved: the swarm and its means are the start, bit for bit
    np.testing.assert_array_equal(got["swarm"], np.repeat(th[:, None], n, axis=1)); np.testing.assert_array_equal(got["theta_mean"][0], th)


def test_a_fixed_slot_keeps_its_bits_and_a_slots_draws_do_not_depend_on_the_others():
    model, data = ragged("c2", 7)
    n, seed = 50, 11
    th = theta_of(model)
    sd = np.zeros(len(th)); sd[[3, 9]] = 0.05                  # mu of the first leaf, sigma of the second
    a = twin_search(model, n, data, sd, 0.5, 3, seed, theta0=th)
    fixed = [j for j in range(len(th)) if sd[j] == 0.0]
    np.testing.assert_array_equal(a["swarm"][fixed], np.repeat(th[fixed, None], n, axis=1))
    np.testing.assert_array_equal(a["theta_mean"][:, fixed], np.repeat(th[None, fixed], 3, axis=0))
    assert np.all(a["swarm"][[3, 9]] != th[[3, 9], None])
    assert np.array_equal(a["theta_mean"], twin_search(model, n, data, sd, 0.5, 3, seed, theta0=th)["theta_mean"])   # one seed, one result
    assert not np.array_equal(a["theta_mean"], twin_search(model, n, data, sd, 0.5, 3, seed + 1, theta0=th)["theta_mean"])
    # without weighing (ancestors = the identity) a slot's walk is its own draws: freeing slots 2 and 4 as well -- 2 shares slot 3's
    # Philox block and its Box-Muller pair -- leaves slot 3 and slot 9 bit for bit what they were; an ivp slot moves once per iteration
    t, y, has = data
    blind = (t, y, np.zeros_like(has))
    b = twin_search(model, n, blind, sd, 0.5, 2, seed, theta0=th)
    sd2 = sd.copy(); sd2[[0, 2, 4]] = 0.07
    c = twin_search(model, n, blind, sd2, 0.5, 2, seed, theta0=th)
    np.testing.assert_array_equal(b["swarm"][[3, 9]], c["swarm"][[3, 9]])
    assert np.all(c["swarm"][[0, 2, 4]] != th[[0, 2, 4], None])
    cool = cooling(0.5, 0, 2)
    tw = build_if2_twin()
    lib = load_library()
    want = th[0]
    for m in range(2):                                          # slot 0 is an m0: perturbed before x0 only
        want = want + (0.07 * cool[m]) * tw.twin_if2_normal(int(lib.cssm_pf_run_key(seed, m + 1)), 5, 0, 0)
    assert c["swarm"][0, 5] == want
    want = th[3]
    for m in range(2):                                          # slot 3 is a mu: before x0 and before each of the 7 records
        for when in range(8):
            want = want + (0.05 * cool[m]) * tw.twin_if2_normal(int(lib.cssm_pf_run_key(seed, m + 1)), 5, when, 3)
    assert c["swarm"][3, 5] == want


def test_a_search_continued_from_its_swarm_is_the_uninterrupted_one_and_a_dead_record_ends_it():
    model, data = ragged("linear", 8)
    th = theta_of(model)
    sd = np.array([0.05, 0.0, 0.0, 0.05])
    whole = twin_search(model, 33, data, sd, 0.3, 4, 5, theta0=th)
    first = twin_search(model, 33, data, sd, 0.3, 1, 5, theta0=th)
    rest = twin_search(model, 33, data, sd, 0.3, 3, 5, swarm0=first["swarm"], first_iter=1)
    np.testing.assert_array_equal(np.vstack([first["theta_mean"], rest["theta_mean"]]), whole["theta_mean"])
    np.testing.assert_array_equal(rest["swarm"], whole["swarm"]); np.testing.assert_array_equal(rest["x"], whole["x"])
    t, y, has = data
    dead = twin_search(model, 33, (t, np.where(np.arange(8) == 5, 1e200, y), has), sd, 0.3, 2, 5, theta0=th)    # every weight is zero
    assert dead["rc"] == _abi.CSSM_ENONFINITE and np.isnan(dead["theta_mean"]).all()
    np.testing.assert_array_equal(dead["swarm"], np.repeat(th[:, None], 33, axis=1))


# 4 ------------------------------------------------------------------------------------------------------------------------------
ACC_T, ACC_N, ACC_M, ACC_COOL = 60, 300, 40, 0.25
ACC_FREE = (0, 3)
ACC_SD = np.array([0.04, 0.0, 0.0, 0.04])
ACC_SEEDS = [9100 + k for k in range(4)]
ACC_STARTS = [(np.log(0.5) + 1.2, np.log(0.3) + 1.5), (np.log(0.5) - 1.2, np.log(0.3) + 1.5), (np.log(0.5) + 1.2, np.log(0.3) - 1.5),
              (np.log(0.5) - 1.2, np.log(0.3) - 1.5)]      # around the values the data were simulated with, far outside the region
CHI2_95_2DOF = 5.99


def acc_data():
    return cases.gaussian_series(ACC_T)


def acc_theta(free):
    th = theta_of(cases.linear_model())
    th[list(ACC_FREE)] = free
    return th


def acc_model(th):
    return _linear_unparam().run(cases.linear_model().parameters().withFlat([float(v) for v in th]))


def _linear_unparam():
    from composablestatespacemodels_amd import Model, Sde
    return Model.linear(Sde.brownianMotion(1))


def kalman_ll(free):
    t, y, has = acc_data()
    return float(gr.kalman(gr.spec_of(acc_model(acc_theta(free))), t, y, has)[0][-1])


_LMAX = None


def l_max():
    """The maximum of the exact log-likelihood over the two free parameters: Nelder-Mead from several starts, the best of them."""
    global _LMAX
    if _LMAX is None:
        from scipy.optimize import minimize
        best = None
        for s in ACC_STARTS + [(np.log(0.5), np.log(0.3))]:
            r = minimize(lambda f: -kalman_ll(f), np.array(s), method="Nelder-Mead", options={"xatol": 1e-7, "fatol": 1e-9, "maxiter": 2000})
            if best is None or r.fun < best.fun:
                best = r
        _LMAX = (-float(best.fun), best.x)
    return _LMAX


def two_delta(free):
    return 2.0 * (l_max()[0] - kalman_ll(free))


def acc_twin(k, blind=False):
    t, y, has = acc_data()
    data = (t, y, np.zeros_like(has) if blind else has)
    return twin_search(cases.linear_model(), ACC_N, data, ACC_SD, ACC_COOL, ACC_M, ACC_SEEDS[k], theta0=acc_theta(ACC_STARTS[k]))


def test_iterated_filtering_reaches_the_likelihood_ratio_region_on_the_twin():
    lmax, at = l_max()
    print(f"    l_max = {lmax:.6f} at (log obs sd, log sigma) = {np.round(at, 4).tolist()}")
    for k, s in enumerate(ACC_STARTS):
        start = two_delta(s)
        got = acc_twin(k)
        hat = got["theta_mean"][-1][list(ACC_FREE)]
        found = two_delta(hat)
        walk = two_delta(acc_twin(k, blind=True)["theta_mean"][-1][list(ACC_FREE)])
        print(f"    search {k}: start 2dl = {start:.2f}; theta_hat = {np.round(hat, 4).tolist()}, 2dl = {found:.3f}; has_obs = 0: 2dl = {walk:.2f}")
        assert got["rc"] == 0
        assert found <= CHI2_95_2DOF, (k, found)                # accepted
        assert start > CHI2_95_2DOF, (k, start)                 # the criterion has power: it rejects where the search began ...
        assert walk > CHI2_95_2DOF, (k, walk)                   # ... and a swarm that only random-walks


# 5 ------------------------------------------------------------------------------------------------------------------------------
class _Recorder:
    """stands where the library stands: keeps what cssm_fleet_if2 was handed and fills the outputs with recognisable values"""

    def __init__(self, S, n, d, nt):
        self.S, self.n, self.d, self.nt, self.calls = S, n, d, nt, []

    def cssm_fleet_if2(self, h, desc, th0, sw0, nt, sd, cool, first, iters, per, seeds, off, t, y, has, mean, ll, swarm, ll_t, ess_t, x, anc, rc):
        o = np.ctypeslib.as_array(off, (self.S + 1,)).copy()
        R = int(o[-1])
        self.calls.append({"off": o, "t": np.ctypeslib.as_array(t, (max(R, 1),)).copy(), "has": np.ctypeslib.as_array(has, (max(R, 1),)).copy(),
                           "theta0": None if th0 is None else np.ctypeslib.as_array(th0, (self.S, nt)).copy(), "swarm0": sw0 is not None,
                           "sd": np.ctypeslib.as_array(sd, (nt,)).copy(), "seeds": np.ctypeslib.as_array(seeds, (self.S,)).copy(),
                           "scalars": (nt, cool, first, iters, per), "opt": (swarm is not None, ll_t is not None, ess_t is not None, x is not None,
                                                                           anc is not None)})
        np.ctypeslib.as_array(mean, (self.S, iters, nt))[:] = np.arange(self.S * iters * nt).reshape(self.S, iters, nt)
        np.ctypeslib.as_array(ll, (self.S, iters))[:] = np.arange(self.S * iters).reshape(self.S, iters) + 0.5
        if ll_t is not None:
            np.ctypeslib.as_array(ll_t, (max(R, 1),))[:R] = np.arange(R) + 0.25
        return 0


def test_what_if2_hands_over_and_how_it_splits_the_rows():
    fl = NativePfFleet.__new__(NativePfFleet)
    fl.S, fl.n, fl.d, fl.n_theta, fl.generation, fl._h, fl.seeds = 3, 10, 2, 4, 0, C.c_void_p(), [0] * 3
    fl.lib = _Recorder(3, 10, 2, 4)
    datas = [(np.arange(3.0), np.ones(3), None), (np.zeros(0), np.zeros(0), None), (np.array([5.0, 6.0]), np.array([2.0, 1.0]), np.array([0, 1]))]
    desc = cases.linear_model().descriptor()
    th0 = np.arange(12.0).reshape(3, 4)
    out = fl.if2(desc, datas, [0.1, 0, 0, 0.2], 0.5, 5, [1, 2, 2**64 + 3], theta0=th0, iters_per_launch=2, want_last=True)
    call = fl.lib.calls[0]
    assert list(call["off"]) == [0, 3, 3, 5] and list(call["t"]) == [0, 1, 2, 5, 6] and list(call["has"]) == [1, 1, 1, 0, 1]
    np.testing.assert_array_equal(call["theta0"], th0)
    assert not call["swarm0"] and list(call["sd"]) == [0.1, 0, 0, 0.2] and list(call["seeds"]) == [1, 2, 3]
    assert call["scalars"] == (4, 0.5, 0, 5, 2) and call["opt"] == (False, True, True, True, True)
    assert out["theta_mean"].shape == (3, 5, 4) and out["ll"][2, 4] == 14.5 and not out["rc"].any() and "swarm" not in out
    assert [list(v) for v in out["ll_t"]] == [[0.25, 1.25, 2.25], [], [3.25, 4.25]] and out["x"].shape == (3, 2, 10)
    out = fl.if2(desc, datas, [0.1, 0, 0, 0.2], 0.5, 5, [1, 2, 3], swarm0=np.zeros((3, 4, 10)), first_iter=7, want_swarm=True)
    call = fl.lib.calls[1]
    assert call["swarm0"] and call["theta0"] is None and call["scalars"] == (4, 0.5, 7, 5, 0) and call["opt"] == (True, False, False, False, False)
    assert out["swarm"].shape == (3, 4, 10) and "ll_t" not in out
    for bad, word in (({"datas": datas[:2]}, "per series"), ({"rw_sd": [0.1, 0.2]}, "n_theta = 4"), ({"seeds": [1, 2]}, "one seed per series")):
        kw = {"datas": datas, "rw_sd": [0.1, 0, 0, 0.2], "seeds": [1, 2, 3], **bad}
        with pytest.raises(ValueError, match=word):
            fl.if2(desc, kw["datas"], kw["rw_sd"], 0.5, 5, kw["seeds"], theta0=th0)
    with pytest.raises(ValueError, match="theta0 .* or swarm0"):
        fl.if2(desc, datas, [0.1, 0, 0, 0.2], 0.5, 5, [1, 2, 3])
    assert len(fl.lib.calls) == 2


def test_the_package_exports_the_search_and_its_result_rebuilds_the_parameters():
    import composablestatespacemodels_amd as pkg
    from composablestatespacemodels_amd.if2 import If2Result
    assert pkg.IF2 is not None and "IF2" in pkg.__all__
    starts = [cases.linear_model().parameters()] * 2
    mean = np.arange(2 * 3 * 4, dtype=np.float64).reshape(2, 3, 4)
    res = If2Result(starts, {"theta_mean": mean, "ll": np.zeros((2, 3)), "rc": np.zeros(2, dtype=np.int32), "swarm": np.zeros((2, 4, 5))})
    assert res.parameters(1).flattenParams() == [20.0, 21.0, 22.0, 23.0]


def test_the_kernel_is_instantiated_per_dimension_and_tested_over_all_sixteen():
    """The rule tests/test_fleet_matrix_host.py and tests/test_fleet_smooth_host.py hold the other fleet kernels to: the kernel is
    dispatched over the latent dimension, and one GPU test runs cases.dim_model(d) for d = 1 .. 16 through the call."""
    import importlib
    import inspect
    src = open(os.path.join(ROOT, "composablestatespacemodels_amd", "csrc", "cssm_fleet_if2.hip")).read()
    assert set(re.findall(r"__global__[^;{]*?void\s+(k_fleet_\w+)\(", src)) == {"k_fleet_if2"}
    assert re.findall(r"hipLaunchKernelGGL\(\(?(k_fleet_\w+)<D", src) == ["k_fleet_if2"] and len(re.findall(r"DISPATCH_D\(", src)) == 1
    mod = importlib.import_module("test_gpu_fleet_if2")
    fn = mod.test_every_latent_dimension
    marks = [m for m in fn.pytestmark if m.name == "parametrize" and m.args[0] == "d"]
    assert marks and list(marks[0].args[1]) == list(range(1, 17))
    body = inspect.getsource(fn)
    assert "cases.dim_model(d)" in body and ".if2(" in body
    assert any(m.name == "gpu" for m in (mod.pytestmark if isinstance(mod.pytestmark, list) else [mod.pytestmark]))
    assert {1, 2, 63, 64, 65, 100, 257, 1000, 2049, 4095, 4096} <= {n for name, n in mod.CASES if name == "c2"}
