"""CPU-only checks of whole PMMH chains for LGCP fleets (include/cssm_pf.h: cssm_fleet_pmmh_chains_lgcp, cssm_fleet_pmmh_lgcp_pack_record):

  * the sequential twin (tests/pmmh_chain_twin.run_chain over tests/pmmh_lgcp_twin.lgcp_ll_fn): with every prior flat and L = sqrt(delta) I
    it is the oracle's pmmh over FilterLgcp bit for bit, which ties the twin to the oracle;
  * every refusal that is made before the fleet is looked at, with its code and the entry point it names;
  * the theta-independent record of an event against the LGCP fleet's own record of the same event;
  * the bindings against the header.

There is no statistical acceptance test here: no exact LGCP likelihood exists to hold a posterior to.  The decision logic is run_chain's,
which tests/test_pmmh_chains_host.py holds to a quadrature; the LGCP filter is held to the oracle in tests/test_gpu_fleet_lgcp.py."""
import ctypes as C
import math
import os
import re
import struct

import numpy as np
import pytest

import cases
import pmmh_lgcp_twin as lt
from composablestatespacemodels_amd import _abi, load_library
from composablestatespacemodels_amd.pmmh import Prior
from oracle import oracle
from test_fleet_lgcp_host import lgcp_record

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A, D_ = _abi.CSSM_EINVAL_ARG, _abi.CSSM_EINVAL_DESC
_dp, _u8p, _u32p, _u64p, _i32p = (C.POINTER(t) for t in (C.c_double, C.c_uint8, C.c_uint32, C.c_uint64, C.c_int32))
CALL = b"cssm_fleet_pmmh_chains_lgcp"


# 1 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["c4", "seasonal"])
def test_flat_priors_and_an_isotropic_factor_are_the_oracles_pmmh(name):
    model = lt.MODELS[name]()
    params = model.parameters()
    theta0 = np.array(params.flattenParams())
    nt = len(theta0)
    assert (model.dimension, nt) == ((1, 5) if name == "c4" else (3, 11))
    t = lt.stream30()
    assert len(t) == 30 and np.any(np.diff(t) == 0.0) and t.min() >= 0.0 and t.max() <= 3.0
    n, iters, delta, seed = 100, 12, 0.3, cases.SEED + 41
    desc = model.descriptor(lt.PRECISION)
    o = oracle.OraclePf(desc, n, 1)
    want = o.pmmh(desc, theta0, delta, *lt.events(t), seed=seed, n_iters=iters)
    ll_fn = lt.lgcp_ll_fn(lt.unparam_of(model), params, n, t)
    got = lt.run_chain(ll_fn, theta0, math.sqrt(delta) * np.eye(nt), None, seed, iters, model.dimension)
    for g, w, what in zip(got, want, ("ll", "theta", "accepted", "last_state")):
        np.testing.assert_array_equal(g, w, err_msg=what)
    print(f"    {name}: accepted {got[2].tolist()}")
    assert got[4].tolist() == [0, 0]
    assert 0 < got[2][-1] < iters                                 # both branches of the decision ran


# 2 ------------------------------------------------------------------------------------------------------------------------------
def _call(lib, desc=None, null=(), off=(0, 2), n_theta=5, chol=None, per_chain=0, priors=None, first=0, iters=2):
    desc = cases.c4_model().descriptor(2) if desc is None else desc
    nt = max(n_theta, 1)
    arr = {"theta0": np.zeros(nt), "chol": np.ascontiguousarray(0.1 * np.eye(nt) if chol is None else chol, dtype=np.float64),
           "seeds": np.zeros(1, dtype=np.uint64), "off": np.asarray(off, dtype=np.uint64), "t": np.arange(4.0),
           "ll": np.zeros(max(iters, 1)), "theta": np.zeros(max(iters, 1) * nt), "acc": np.zeros(max(iters, 1), dtype=np.int32),
           "last": np.zeros(max(iters, 1) * 16), "rc": np.zeros(1, dtype=np.int32)}
    p = lambda name, ty: None if name in null else arr[name].ctypes.data_as(ty)
    pri = None if priors is None else (_abi.Prior * len(priors))(*priors)
    return lib.cssm_fleet_pmmh_chains_lgcp(None, None if "desc" in null else desc.ptr(), p("theta0", _dp), n_theta, p("chol", _dp), per_chain, pri,
                                           None, None, first, iters, 0, p("seeds", _u64p), p("off", _u64p), p("t", _dp), p("ll", _dp),
                                           p("theta", _dp), p("acc", _i32p), p("last", _dp), None, p("rc", C.POINTER(C.c_int)))


def test_whole_call_refusals_are_made_before_the_fleet_is_looked_at():
    lib = load_library()
    err = lambda: lib.cssm_last_error()
    for name in ("desc", "theta0", "chol", "seeds", "off"):
        assert _call(lib, null=(name,)) == A and b"null argument" in err() and CALL in err(), name
    for name in ("ll", "theta", "acc", "last", "rc"):
        assert _call(lib, null=(name,)) == A and b"null output" in err() and CALL in err(), name
    assert _call(lib, off=(1, 2)) == A and b"off[0] must be 0" in err()
    assert _call(lib, null=("t",)) == A and b"null data" in err()
    # a descriptor that is not LGCP: sent to the call that serves it
    assert _call(lib, desc=cases.linear_model().descriptor(), n_theta=4) == D_ and CALL in err() and b"cssm_fleet_pmmh_chains serves" in err()
    assert _call(lib, desc=cases.c2_model().descriptor(), n_theta=10) == D_ and b"cssm_fleet_pmmh_chains serves" in err()
    for bad in (4, 6):
        assert _call(lib, n_theta=bad) == A and b"the descriptor flattens to 5" in err() and CALL in err(), bad
    for bad in (np.nan, np.inf, -np.inf):
        L = 0.1 * np.eye(5); L[2, 1] = bad
        assert _call(lib, chol=L) == A and b"[2][1] is not finite" in err() and CALL in err(), bad
    L = 0.1 * np.eye(5); L[1, 3] = 1e-300
    assert _call(lib, chol=L) == A and b"[1][3]" in err() and b"above the diagonal" in err() and CALL in err()
    L = np.tril(np.ones((5, 5))); L[2, :] = 0.0                                              # a full lower triangle with a zero row is fine
    assert _call(lib, chol=L) == A and b"null fleet" in err()
    flat = [Prior.flat()] * 5
    for bad, words in ((Prior.normal(0.0, 0.0), b"sd > 0"), (Prior.normal(0.0, -1.0), b"sd > 0"), (Prior.normal(0.0, np.inf), b"sd > 0"),
                       (Prior.normal(0.0, np.nan), b"sd > 0"), (Prior.normal(np.nan, 1.0), b"finite mean"), (Prior.uniform(1.0, 0.5), b"a <= b"),
                       (Prior.uniform(np.nan, 0.5), b"a <= b"), (_abi.Prior(3, 0, 0.0, 1.0), b"unknown kind 3"), (_abi.Prior(-1, 0, 0.0, 1.0), b"unknown kind")):
        assert _call(lib, priors=flat[:2] + [bad] + flat[3:]) == A and b"priors[2]" in err() and words in err() and CALL in err(), (bad.kind, bad.a, bad.b)
    ok = [Prior.normal(0.0, 1.0), Prior.uniform(-np.inf, np.inf), Prior.uniform(2.0, 2.0), Prior.flat(), Prior.flat()]
    assert _call(lib, priors=ok) == A and b"null fleet" in err()
    for bad in (0, 1000001):
        assert _call(lib, iters=bad) == A and b"n_iters must be in [1, 1000000]" in err() and CALL in err(), bad
    assert _call(lib, first=2**31 - 1, iters=2) == A and b"first_iter + n_iters" in err() and CALL in err()
    assert _call(lib, first=2**31 - 2, iters=2) == A and b"null fleet" in err()
    # every earlier refusal wins over the later ones; the last one made without a fleet is the fleet's absence
    assert _call(lib, off=(1, 2), iters=0, n_theta=3) == A and b"off[0] must be 0" in err()
    assert _call(lib, desc=cases.linear_model().descriptor(), n_theta=3, iters=0) == D_
    assert _call(lib) == A and b"null fleet" in err()
    ms = np.full(1, 7.0)
    assert lib.cssm_fleet_pmmh_chains_lgcp_last_ms(None, ms.ctypes.data_as(_dp)) == A and ms[0] == 7.0


# 3 ------------------------------------------------------------------------------------------------------------------------------
def pmmh_record(model, precision, t_prev, t, step, fsub_cap=1 << 16):
    """(d, (dt, n_sub, step, fsub_off, pad), fco[d], table rows [n_sub][d] or an empty array, rc)"""
    lib = load_library()
    buf, nb, nf = (C.c_uint8 * 1024)(), C.c_size_t(), C.c_size_t()
    tab = np.zeros(max(fsub_cap, 1))
    rc = lib.cssm_fleet_pmmh_lgcp_pack_record(model.descriptor(precision).ptr(), t_prev, t, step, buf, 1024, C.byref(nb),
                                              tab.ctypes.data_as(_dp) if fsub_cap else None, fsub_cap, C.byref(nf))
    if rc:
        return None, None, None, nf.value, rc
    raw = bytes(buf[:nb.value])
    d = (nb.value - 24) // 8
    assert nb.value == 24 + 8 * d
    return d, struct.unpack("<diIII", raw[:24]), np.frombuffer(raw[24:], dtype=np.float64), tab[:nf.value].reshape(-1, d), rc


@pytest.mark.parametrize("name", ["c4", "seasonal"])
def test_the_record_is_the_theta_independent_part_of_the_lgcp_fleets(name):
    model = lt.MODELS[name]()
    dim = model.dimension
    rng = np.random.default_rng(cases.SEED + 5 + len(name))
    pairs = [(4.5, 4.5, 3), (0.0, 0.0, 0)]                        # an event at the time of the one before: n_sub == 0
    for _ in range(8):
        tp = float(np.round(rng.uniform(0, 30), 3))
        pairs.append((tp, tp + float(rng.choice([0.01, 0.25, 0.3, 1.0, np.round(rng.uniform(0.001, 3), 3)])), int(rng.integers(0, 1000))))
    for precision in (1, 2):
        for t_prev, t, step in pairs:
            d, (dt, n_sub, step_r, fsub_off, pad), fco, rows, rc = pmmh_record(model, precision, t_prev, t, step)
            assert rc == 0 and d == dim
            fd, (_, fdt, fn_sub, fstep, ffsub_off, _), fcoef, ffco, frows = lgcp_record(model, precision, 1000, 99, t_prev, t, step)
            assert fd == d and 24 + 8 * d < 32 + 40 * d
            assert (dt, n_sub, step_r, fsub_off, pad) == (fdt, fn_sub, fstep, ffsub_off, 0)
            np.testing.assert_array_equal(fco, ffco)
            np.testing.assert_array_equal(rows, frows)
            if t == t_prev:
                assert n_sub == 0 and dt == 0.0 and rows.size == 0
            else:
                assert n_sub >= 1 and dt == 10.0 ** -precision and rows.shape == ((n_sub, d) if name == "seasonal" else (0, d))
    # the sizes: 24 + 8 d against 32 + 40 d
    assert 24 + 8 * dim == (32 if name == "c4" else 48)
    lib = load_library()
    buf, nb, nf = (C.c_uint8 * 1024)(), C.c_size_t(), C.c_size_t()
    # what it refuses: another observation model, a buffer or a table that is too small (said with the size)
    assert lib.cssm_fleet_pmmh_lgcp_pack_record(cases.c2_model().descriptor().ptr(), 0.0, 1.0, 0, buf, 1024, C.byref(nb), None, 0, C.byref(nf)) == D_
    assert lib.cssm_fleet_pmmh_lgcp_pack_record(model.descriptor(1).ptr(), 0.0, 1.0, 0, buf, 23 + 8 * dim, C.byref(nb), None, 0, C.byref(nf)) == A
    assert nb.value == 24 + 8 * dim
    assert lib.cssm_fleet_pmmh_lgcp_pack_record(model.descriptor(1).ptr(), 0.0, 1.0, 0, None, 1024, C.byref(nb), None, 0, C.byref(nf)) == A
    if name == "seasonal":
        *_, need, rc = pmmh_record(model, 1, 0.0, 1.0, 0, fsub_cap=0)
        assert rc == A and need == 10 * 3


# 4 ------------------------------------------------------------------------------------------------------------------------------
def test_the_calls_are_bound_exported_and_declared_as_bound():
    lib = load_library()
    sig = {s[0]: s for s in _abi.SYMBOLS}
    header = open(os.path.join(ROOT, "include", "cssm_pf.h")).read()
    ctype = {"cssm_fleet*": C.c_void_p, "const cssm_model_desc*": _abi._descp, "const double*": _dp, "double*": _dp, "const uint64_t*": _u64p,
             "uint32_t*": _u32p, "int32_t*": _i32p, "int*": C.POINTER(C.c_int), "double": C.c_double, "uint32_t": C.c_uint32,
             "size_t": C.c_size_t, "int": C.c_int, "const void*": C.c_void_p, "unsigned char*": _u8p, "size_t*": C.POINTER(C.c_size_t)}
    for name in ("cssm_fleet_pmmh_chains_lgcp", "cssm_fleet_pmmh_chains_lgcp_last_ms", "cssm_fleet_pmmh_lgcp_pack_record"):
        assert name in sig and hasattr(lib, name)
        m = re.search(r"\bint " + name + r"\(([^)]*)\);", header)
        assert m, f"{name} is not declared in include/cssm_pf.h"
        args = [" ".join(a.split()[:-1]) for a in m.group(1).replace("\n", " ").split(",")]
        assert [ctype[a] for a in args] == list(sig[name][2]), (name, args)
    # the plain call's arguments without y and has_obs
    plain, lgcp = list(sig["cssm_fleet_pmmh_chains"][2]), list(sig["cssm_fleet_pmmh_chains_lgcp"][2])
    assert plain[:15] + plain[17:] == lgcp
    numerics = open(os.path.join(ROOT, "include", "cssm_numerics.h")).read()
    assert numerics.count("PMMH chains on the device: LGCP.") == 1
    assert numerics.index("PMMH chains on the device: LGCP.") > numerics.index("---- PMMH chains on the device */")
    import composablestatespacemodels_amd as pkg
    from composablestatespacemodels_amd import pmmh
    from composablestatespacemodels_amd.filter import NativeLgcpFleet, NativePfFleet
    assert pkg.pmmh_lgcp_fleet_chains is pmmh.pmmh_lgcp_fleet_chains and "pmmh_lgcp_fleet_chains" in pkg.__all__
    assert hasattr(NativeLgcpFleet, "pmmh_chains_lgcp") and hasattr(NativeLgcpFleet, "pmmh_chains_lgcp_last_ms")
    assert not hasattr(NativePfFleet, "pmmh_chains_lgcp") and NativeLgcpFleet.pmmh_chains is NativePfFleet.pmmh_chains
    assert pmmh.LGCP_ITERS_PER_LAUNCH == 100
