"""CPU-only checks of the fleet filter's host side (include/cssm_pf.h: cssm_fleet_*): the ctypes view matches the header, the ragged
packing of NativePfFleet.ll_filter, refusals that need no device, the key derivation of FilterFleet, pilotRun's variance, and the
compact per-observation record the fleet uploads against cssm_build_rec's fields (recomputed here through the oracle's contract
functions and the library's own single-observation entry points)."""
import ctypes as C
import os
import re
import struct

import numpy as np
import pytest

import cases
from composablestatespacemodels_amd import CssmError, Streaming, _abi, load_library
from composablestatespacemodels_amd.filter import FilterFleet, NativePfFleet, Resampling
from oracle import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_CTYPES = {"int": C.c_int, "void": None, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "double": C.c_double, "size_t": C.c_size_t}


def _ctype_of(decl):
    """ctypes type of one C parameter / return declaration of the fleet section (pointers to the scalar types, handles, descriptors)"""
    decl = re.sub(r"\bconst\b", "", decl).strip()
    stars = decl.count("*")
    base = decl.replace("*", " ").split()
    base = base[0] if base[0] != "unsigned" else " ".join(base[:2])
    if base in ("cssm_fleet",):
        return C.c_void_p if stars == 1 else C.POINTER(C.c_void_p)
    if base == "cssm_model_desc":
        return C.POINTER(_abi.ModelDesc) if stars == 1 else C.POINTER(C.POINTER(_abi.ModelDesc))
    ty = {"uint8_t": C.c_uint8, "int32_t": C.c_int32, "unsigned char": C.c_uint8, **_CTYPES}[base]
    for _ in range(stars):
        ty = C.POINTER(ty)
    return ty


def test_ctypes_signatures_match_the_header():
    src = open(os.path.join(ROOT, "include", "cssm_pf.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    decls = re.findall(r"^\s*([A-Za-z_][\w\s\*]*?)\b(cssm_fleet_\w+)\s*\(([^;]*?)\)\s*;", src, flags=re.M)
    bound = {s[0]: s for s in _abi.SYMBOLS if s[0].startswith("cssm_fleet_")}
    assert {d[1] for d in decls} == set(bound) and len(bound) >= 15
    for ret, name, args in decls:
        want_args = [_ctype_of(re.sub(r"\b\w+$", "", a.strip()) if not a.strip().endswith("*") else a) for a in args.split(",")]
        _, res, got = bound[name]
        assert res == _ctype_of(ret), name
        assert [g for g in got] == want_args, (name, got, want_args)
    lib = load_library()
    assert _abi.FLEET_MAX_N == int(re.search(r"#define CSSM_FLEET_MAX_N (\d+)", src).group(1)) == 4096
    for name in bound:
        assert hasattr(lib, name)


def test_ragged_packing():
    a = (np.arange(3.0), [1, 2, 3], None)
    b = (np.array([5.0, 4.0], dtype=np.float32), np.array([7, 8], dtype=np.int64), [1, 0])
    c = (np.arange(10.0)[::2], np.arange(10.0)[::2] * 2, np.ones(5, dtype=bool))       # non-contiguous views
    off, t, y, has = NativePfFleet.pack([a, b, c])
    assert off.dtype == np.uint64 and list(off) == [0, 3, 5, 10]
    assert t.dtype == np.float64 and y.dtype == np.float64 and has.dtype == np.uint8
    assert t.flags.c_contiguous and y.flags.c_contiguous and has.flags.c_contiguous
    assert list(t) == [0, 1, 2, 5, 4, 0, 2, 4, 6, 8] and list(y) == [1, 2, 3, 7, 8, 0, 4, 8, 12, 16]
    assert list(has) == [1, 1, 1, 1, 0, 1, 1, 1, 1, 1]
    with pytest.raises(ValueError, match="series 1 has no records"):
        NativePfFleet.pack([a, (np.zeros(0), np.zeros(0), None)])
    with pytest.raises(ValueError, match="differ in length"):
        NativePfFleet.pack([(np.zeros(2), np.zeros(3), None)])


def test_an_empty_series_is_rejected_before_any_device_call():
    """ll_filter packs (and refuses) before it touches the handle: a fleet object without a handle shows it."""
    fl = NativePfFleet.__new__(NativePfFleet)
    fl.S, fl.n, fl.d, fl.generation, fl._h, fl.lib = 2, 10, 1, 0, C.c_void_p(), None
    with pytest.raises(ValueError, match="no records"):
        fl.ll_filter([(np.zeros(2), np.zeros(2), None), (np.zeros(0), np.zeros(0), None)])
    with pytest.raises(ValueError, match="one .* per series"):
        fl.ll_filter([(np.zeros(2), np.zeros(2), None)])


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="this check is for hosts without a GPU")
def test_no_device_is_ehip_with_the_usual_message():
    lib = load_library()
    h = C.c_void_p()
    rc = lib.cssm_fleet_create(cases.c2_model().descriptor().ptr(), 100, 4, 0, C.byref(h))
    assert rc == _abi.CSSM_EHIP and not h.value
    assert b"no CPU path" in lib.cssm_last_error()
    with pytest.raises(CssmError):
        FilterFleet([cases.c1_model()] * 2, Resampling.systematicResampling, 100)
    with pytest.raises(CssmError):
        Streaming.pilotRun([], cases.c1_model(), [100], 4)


def test_argument_refusals_come_before_the_device():
    lib = load_library()
    h = C.c_void_p()
    d = cases.c2_model().descriptor()
    for n, s, code, word in ((0, 2, _abi.CSSM_EINVAL_ARG, b"particles"), (_abi.FLEET_MAX_N + 1, 2, _abi.CSSM_EINVAL_ARG, b"cssm_pfb_"),
                             (100, 0, _abi.CSSM_EINVAL_ARG, b"series")):
        assert lib.cssm_fleet_create(d.ptr(), n, s, 0, C.byref(h)) == code and not h.value
        assert word in lib.cssm_last_error()
    assert lib.cssm_fleet_create(cases.c4_model().descriptor(2).ptr(), 100, 2, 0, C.byref(h)) == _abi.CSSM_EINVAL_DESC
    assert b"LGCP" in lib.cssm_last_error() and b"cssm_pf_" in lib.cssm_last_error()


def test_filter_fleet_keys_are_run_keys():
    lib = load_library()
    keys = FilterFleet.keys(cases.SEED, 5)
    assert keys == [int(lib.cssm_pf_run_key(cases.SEED, k)) for k in range(5)]
    assert keys == [int(oracle.lib().oracle_c_derive_key(cases.SEED, k)) for k in range(5)]
    assert len(set(keys)) == 5 and all(k != cases.SEED + i for i, k in enumerate(keys))      # never seed + k


def test_pilot_run_variance_on_injected_log_likelihoods():
    rng = np.random.default_rng(3)
    table = {n: rng.standard_normal(7) * s - 100.0 for n, s in ((100, 1.0), (400, 0.5), (1600, 0.2))}
    seen = []

    def ll_fn(n, keys):
        seen.append((n, list(keys)))
        return table[n]

    out = Streaming.pilotRun([], cases.c1_model(), (400, 100, 1600), 7, seed=11, ll_fn=ll_fn)
    assert [n for n, _ in out] == [400, 100, 1600]                                          # in the order given
    for n, v in out:
        assert v == float(np.var(table[n], ddof=1))
    assert all(k == FilterFleet.keys(11, 7) for _, k in seen)
    with pytest.raises(ValueError):
        Streaming.pilotRun([], cases.c1_model(), (100,), 1, ll_fn=ll_fn)


# ---- the compact record ------------------------------------------------------------------------------------------------------------
_MODELS = ["c1", "c2", "c3", "linear", "negbin", "zip", "bernoulli", "studentt", "beta", "gbsg", "euler"]


def _record(model, n, seed, t_prev, t, y, has, step):
    lib = load_library()
    buf = (C.c_uint8 * 1024)()
    nb = C.c_size_t()
    assert lib.cssm_fleet_pack_record(model.descriptor().ptr(), n, seed, t_prev, t, y, has, step, buf, 1024, C.byref(nb)) == 0
    raw = bytes(buf[:nb.value])
    d = (nb.value - 80) // 40
    assert nb.value == 80 + 40 * d
    head = struct.unpack("<9diI", raw[:80])
    tail = np.frombuffer(raw[80:], dtype=np.float64)
    return d, head, tail[:4 * d].reshape(d, 4), tail[4 * d:]


@pytest.mark.parametrize("name", _MODELS)
def test_compact_record_holds_the_fields_the_step_uses(name):
    """Random (t_prev, t, y) per model: the record's uniform, level, time increment, observation constants and coefficients against the
    same quantities recomputed independently -- the oracle's contract functions (uniform, level), its constrained components and the
    closed-form transition moments (coefficients), the seasonal phase (f coefficients)."""
    model = cases.literal_case(name, 4)[0]
    rng = np.random.default_rng(cases.SEED + len(name))
    n, seed = 1000, 123456789
    o = oracle.OraclePf(model.descriptor(), n, seed)
    comp = o.components()                                    # [d][5] = m0, c0, mu, phi, sigma, constrained
    kinds = [l.sde_kind for l in (model.descriptor().desc.leaves[i] for i in range(model.descriptor().desc.n_leaves)) for _ in range(l.dim)]
    for trial in range(20):
        t_prev = float(rng.uniform(0, 50)); t = t_prev + float(rng.choice([0.25, 1.0, 3.5, rng.uniform(0.01, 5)]))
        y = float(rng.integers(0, 9)) if model.obs_kind in (_abi.OBS_POISSON, _abi.OBS_NEGBIN, _abi.OBS_ZIP) else float(rng.uniform(0.05, 0.95))
        has, step = int(rng.integers(0, 2)), int(rng.integers(0, 1000))
        d, head, coef, fco = _record(model, n, seed, t_prev, t, y, has, step)
        assert d == o.d
        yy, c0, c1, c2, c3, cdf, u, dt, ref, has_r, step_r = head
        assert (has_r, step_r) == (has, step) and dt == t - t_prev and yy == y
        assert 0.0 <= u < 1.0
        assert ref == o.ref_level(y) or (np.isnan(ref) and np.isnan(o.ref_level(y)))
        for k in range(d):
            m0, c0k, mu, phi, sigma = comp[k]
            if kinds[k] == _abi.SDE_BROWNIAN:
                want = [0.0, 0.0, 0.0, np.sqrt(sigma * dt)]
            elif kinds[k] == _abi.SDE_GEN_BROWNIAN:
                want = [mu * dt, 0.0, 0.0, np.sqrt(sigma * dt)]
            elif kinds[k] == _abi.SDE_OU:
                want = [mu, float(oracle.c_exp([-phi * dt])[0]), 0.0, np.sqrt((sigma * sigma / (phi * 2.0)) * (1.0 - float(oracle.c_exp([phi * -2.0 * dt])[0])))]
            else:
                want = [mu, phi, sigma, np.sqrt(dt)]
            assert list(coef[k]) == want, (k, list(coef[k]), want)
        assert np.all(np.abs(fco) <= 1.0)
    # the same observation packed twice gives the same bytes; another key moves only the uniform
    a = _record(model, n, seed, 1.0, 2.0, 1.0, 1, 3); b = _record(model, n, seed, 1.0, 2.0, 1.0, 1, 3); c = _record(model, n, seed + 1, 1.0, 2.0, 1.0, 1, 3)
    assert a[1] == b[1] and a[1][6] != c[1][6] and a[1][:6] == c[1][:6] and np.array_equal(a[2], c[2])
