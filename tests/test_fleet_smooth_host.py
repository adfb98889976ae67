"""CPU-only checks of the fleet's backward-simulation smoother (include/cssm_pf.h: cssm_fleet_smooth, cssm_fleet_smooth_last_ms; an
EXTENSION -- the reference has no smoother beyond FilterInterpolate):

  * the sequential twin of the contract's backward simulation (tests/cpp/backsim_twin.c, written from include/cssm_numerics.h alone) on
    hand-worked cases, and against an independent float numpy statement of the backward kernel on an oracle forward pass: per row the
    frequencies of the particles the twin picks over many keys against the closed-form probabilities p(i) proportional to exp(lb_i), by
    a chi-square test at level 1e-4 with fixed seeds (a deterministic test: the level says how surprising the fixed outcome may be);
  * the bindings against the header, the refusals that are made before the fleet is looked at, and what the Python side hands over.

The helpers that build the twin and an oracle history are imported by the GPU files (tests/test_gpu_fleet_smooth*.py)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
from scipy.stats import chi2

import cases
from composablestatespacemodels_amd import Data, _abi, load_library
from composablestatespacemodels_amd.filter import FilterFleet, NativePfFleet
from oracle import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A = _abi.CSSM_EINVAL_ARG
_dp, _u8p, _u32p, _u64p, _i32p = (C.POINTER(t) for t in (C.c_double, C.c_uint8, C.c_uint32, C.c_uint64, C.c_int32))
_TWIN = None


def build_backsim_twin(out_dir=None) -> C.CDLL:
    """tests/cpp/backsim_twin.c built with the gcc line of the other twins (once per process)."""
    global _TWIN
    if _TWIN is None:
        import tempfile
        so = os.path.join(str(out_dir or tempfile.mkdtemp(prefix="backsim_twin_")), "backsim_twin.so")
        subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-mfma", "-std=c99", "-shared", "-fPIC", "-o", so,
                               os.path.join(ROOT, "tests", "cpp", "backsim_twin.c"), "-lm"])
        lib = C.CDLL(so)
        lib.twin_backsim.argtypes = [_dp, _u32p, _u8p, _i32p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, _u32p]
        lib.twin_backsim.restype = C.c_int
        lib.twin_back_uniform.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32]
        lib.twin_back_uniform.restype = C.c_double
        lib.twin_back_start.argtypes = [C.c_uint32] * 3
        lib.twin_back_start.restype = C.c_uint32
        _TWIN = lib
    return _TWIN


def twin_traj(X, Anc, recs, kinds, seed, M) -> np.ndarray:
    """traj[T + 1, M] of the twin on a history X[T + 1, d, n], Anc[T + 1, n] and the T records' bytes."""
    X = np.ascontiguousarray(X, dtype=np.float64); Anc = np.ascontiguousarray(Anc, dtype=np.uint32)
    recs = np.ascontiguousarray(recs, dtype=np.uint8); kinds = np.ascontiguousarray(kinds, dtype=np.int32)
    T1, d, n = X.shape
    assert Anc.shape == (T1, n) and recs.size == (T1 - 1) * (80 + 40 * d) and kinds.shape == (d,) and T1 >= 2
    out = np.zeros((T1, M), dtype=np.uint32)
    rc = build_backsim_twin().twin_backsim(X.ctypes.data_as(_dp), Anc.ctypes.data_as(_u32p), recs.ctypes.data_as(_u8p), kinds.ctypes.data_as(_i32p),
                                           int(seed) & (2**64 - 1), n, int(M), T1 - 1, d, out.ctypes.data_as(_u32p))
    assert rc == 0
    return out


def kinds_of(model) -> np.ndarray:
    """CSSM_SDE_* of every latent component, from cssm_model_structure (bits 0..1 of a component's byte)."""
    words = (C.c_uint32 * (_abi.MAX_DIM // 4))()
    d = C.c_int32()
    _abi.check(load_library().cssm_model_structure(model.descriptor().ptr(), words, C.byref(d)))
    return np.array([(words[k >> 2] >> ((k & 3) * 8)) & 3 for k in range(d.value)], dtype=np.int32)


def pack_records(model, n, seed, t, y, has) -> np.ndarray:
    """The T records of a series as the fleet uploads them (cssm_fleet_pack_record): t_prev = the slice's smallest time, then t[s - 1]."""
    lib = load_library()
    out = []
    tp = float(np.min(t))
    for s in range(len(t)):
        buf = np.zeros(1024, dtype=np.uint8); nb = C.c_size_t()
        _abi.check(lib.cssm_fleet_pack_record(model.descriptor().ptr(), n, int(seed) & (2**64 - 1), tp, float(t[s]), float(y[s]), int(has[s]), s,
                                              buf.ctypes.data_as(_u8p), 1024, C.byref(nb)))
        out.append(buf[:nb.value].copy())
        tp = float(t[s])
    return np.concatenate(out)


def oracle_history(model, n, seed, data):
    """(ll, X[T + 1, d, n], Anc[T + 1, n]) of the oracle stepping through a series: slice 0 the initial cloud, slice s + 1 the cloud
    record s proposed and the ancestors that resampled it (the identity behind an unweighted record).  OracleError where it fails."""
    t, y, has = data
    o = oracle.OraclePf(model.descriptor(), n, seed)
    o.init(float(np.min(t)))
    X, Anc = [o.particles()], [o.ancestors()]
    ll = 0.0
    for s in range(len(t)):
        ll, _ = o.step(float(t[s]), float(y[s]), bool(has[s]))
        X.append(o.proposed()); Anc.append(o.ancestors())
    return ll, np.array(X), np.array(Anc)


def hand_record(d, dt, coef):
    """The bytes of a record with the given dt and coefficients [d][4]; everything the backward pass does not read is zero."""
    r = np.zeros(80 + 40 * d, dtype=np.uint8)
    r[56:64] = np.frombuffer(np.float64(dt).tobytes(), dtype=np.uint8)
    r[80:80 + 32 * d] = np.frombuffer(np.asarray(coef, dtype=np.float64).tobytes(), dtype=np.uint8)
    return r


# 1 ------------------------------------------------------------------------------------------------------------------------------
def test_the_contract_names_the_stream_and_the_twin_states_the_start_and_the_uniform():
    src = open(os.path.join(ROOT, "include", "cssm_numerics.h")).read()
    assert re.search(r"#define CSSM_STREAM_BACK \(11u\)", src)
    others = {int(v) for v in re.findall(r"#define CSSM_STREAM_\w+ (\d+)u", src + open(os.path.join(ROOT, "include", "cssm_obs_draws.h")).read())}
    assert 11 not in others and max(others) == 10           # no other stream of the contract has the tag
    tw = build_backsim_twin()
    for m, n, M in ((0, 5, 3), (1, 5, 3), (2, 5, 3), (4095, 4096, 4096), (6, 1000, 7), (0, 7, 1)):
        assert tw.twin_back_start(m, n, M) == (m * n) // M < n
    ctr = np.array([3, 0, 9, (11 << 28)], dtype=np.uint32); key = np.array([0x89abcdef, 0x01234567], dtype=np.uint32)
    blk = oracle.c_philox_contract(ctr, key)
    want = (int(blk[0]) * 2.0**-32) + ((int(blk[1]) >> 11) * 2.0**-53)
    assert tw.twin_back_uniform(0x0123456789abcdef, 3, 9) == want and 0.0 <= want < 1.0


# 2 ------------------------------------------------------------------------------------------------------------------------------
def test_hand_worked_an_overwhelmingly_closer_parent_wins():
    """N = 2, one Brownian component with sd 1: the other parent is 100 away, its weight exp(-5000) is 0 on the 2^-96 grid, so C = (1, 1)
    or (0, 1) whatever u is."""
    X = np.array([[[0.0, 100.0]], [[0.1, 100.2]]])
    ident = np.array([[0, 1], [0, 1]], dtype=np.uint32)
    rec = hand_record(1, 1.0, [[0.0, 0.0, 0.0, 1.0]])
    for seed in (1, 2, 99):
        np.testing.assert_array_equal(twin_traj(X, ident, rec, [0], seed, 2), [[0, 1], [0, 1]])
        # the final cloud resampled (1, 0): slot 0 holds particle 1, whose parent is particle 1 of slice 0
        np.testing.assert_array_equal(twin_traj(X, np.array([[0, 1], [1, 0]], dtype=np.uint32), rec, [0], seed, 2), [[1, 0], [1, 0]])
        # M = 1 starts in slot 0; M = 4 starts in slots 0, 0, 1, 1
        np.testing.assert_array_equal(twin_traj(X, ident, rec, [0], seed, 4), [[0, 0, 1, 1], [0, 0, 1, 1]])
    # an OU component pulled to p0 = 100 with p1 = 0: both parents have mean 100, the weights are equal, C = (0.5, 1): u decides
    rec = hand_record(1, 1.0, [[100.0, 0.0, 0.0, 1.0]])
    tw = build_backsim_twin()
    for seed in range(20):
        got = twin_traj(X, ident, rec, [2], seed, 2)
        for m in range(2):
            assert got[0, m] == (0 if tw.twin_back_uniform(seed, m, 0) <= 0.5 else 1)


def test_hand_worked_a_record_without_diffusion_follows_the_genealogy():
    """dt = 0 makes p3 = 0: i_s = j_{s+1}, the slot that produced the particle, then j_s = A_s[i_s]."""
    n, T = 4, 3
    rng = np.random.default_rng(3)
    X = rng.normal(size=(T + 1, 1, n))
    Anc = np.array([[0, 1, 2, 3], [2, 2, 0, 1], [3, 0, 0, 1], [1, 1, 2, 0]], dtype=np.uint32)
    recs = np.concatenate([hand_record(1, 0.0, [[0.0, 0.0, 0.0, 0.0]])] * T)
    got = twin_traj(X, Anc, recs, [0], 5, n)
    want = np.zeros((T + 1, n), dtype=np.uint32)
    want[T] = Anc[T]
    for s in range(T - 1, -1, -1):
        want[s] = Anc[s][want[s + 1]]
    np.testing.assert_array_equal(got, want)
    # a NaN diffusion and a zero Euler factor (sd = p2 p3) do the same; a positive one does not have to
    for kind, coef in ((0, [0.0, 0.0, 0.0, np.nan]), (3, [0.0, 0.0, 0.0, 1.0]), (3, [0.0, 0.0, 1.0, 0.0])):
        recs = np.concatenate([hand_record(1, 1.0, [coef])] * T)
        np.testing.assert_array_equal(twin_traj(X, Anc, recs, [kind], 5, n), want)


# 3 ------------------------------------------------------------------------------------------------------------------------------
def _numpy_probabilities(kinds, coef, dt, Xs, As, target):
    """p(slot i) of the backward kernel in plain numpy: the Gaussian transition density from x_s[i] = Xs[:, As[i]] to `target`."""
    x = Xs[:, As]                                              # [d, n]
    lp = np.zeros(x.shape[1])
    for c, kind in enumerate(kinds):
        p0, p1, p2, p3 = coef[c]
        mean = (x[c], x[c] + p0, p0 + (x[c] - p0) * p1, x[c] + (p0 + p1 * x[c]) * dt)[kind]
        sd = p2 * p3 if kind == 3 else p3
        lp += -0.5 * ((target[c] - mean) / sd) ** 2
    p = np.exp(lp - lp.max())
    return p / p.sum()


@pytest.mark.parametrize("name", ["linear", "c2", "euler"])
def test_twin_frequencies_against_the_closed_form(name):
    model = {"linear": cases.linear_model, "c2": cases.c2_model, "euler": cases.euler_model}[name]()
    n, T, K = 12, 4, 1500
    t, y, has = cases.gaussian_series(T, seed=cases.SEED + 1) if name == "linear" else cases.poisson_counts(T, seed=cases.SEED + 1)
    t = t + 0.5 * np.arange(T)                                 # (no repeated time: every step is a draw; t0 = t[0] makes record 0 genealogical)
    _, X, Anc = oracle_history(model, n, cases.SEED, (t, y, has))
    recs = pack_records(model, n, cases.SEED, t, y, has)
    kinds = kinds_of(model)
    d = len(kinds)
    RB = 80 + 40 * d
    trajs = np.array([twin_traj(X, Anc, recs, kinds, 1000 + k, n) for k in range(K)])       # [K, T + 1, n]
    assert trajs.max() < n
    np.testing.assert_array_equal(trajs[:, 0], Anc[0][trajs[:, 1]])   # record 0 has dt = 0: the genealogy
    for s in range(1, T):
        r = recs[s * RB:(s + 1) * RB]
        dt = float(np.frombuffer(r[56:64].tobytes())[0])
        coef = np.frombuffer(r[80:80 + 32 * d].tobytes()).reshape(d, 4)
        assert dt > 0
        # the uniforms of index s are independent of the particle held at s + 1: expected counts = the sum of the conditional laws
        expect = np.zeros(n)
        cache = {}
        for j in np.unique(trajs[:, s + 1]):
            p_slot = _numpy_probabilities(kinds, coef, dt, X[s], Anc[s], X[s + 1][:, j])
            cache[j] = np.bincount(Anc[s], weights=p_slot, minlength=n)          # particle = A_s[slot]
            expect += cache[j] * np.count_nonzero(trajs[:, s + 1] == j)
        seen = np.bincount(trajs[:, s].ravel(), minlength=n).astype(float)
        assert seen.sum() == expect.sum().round() == K * n
        big = expect >= 5.0                                    # pool the rare particles into one bin
        ob = np.append(seen[big], seen[~big].sum()); ex = np.append(expect[big], expect[~big].sum())
        keep = ex > 0
        stat = float((((ob - ex) ** 2)[keep] / ex[keep]).sum())
        dof = int(keep.sum()) - 1
        p = float(chi2.sf(stat, dof)) if dof > 0 else 1.0
        print(f"    {name} row {s}: chi2 {stat:.1f} on {dof} dof, p = {p:.3g}")
        assert seen[expect == 0].sum() == 0 and p > 1e-4, (name, s, stat, dof, p)


# 4 ------------------------------------------------------------------------------------------------------------------------------
def test_the_calls_are_bound_exported_and_declared_as_bound():
    lib = load_library()
    sig = {s[0]: s for s in _abi.SYMBOLS}
    header = open(os.path.join(ROOT, "include", "cssm_pf.h")).read()
    ctype = {"cssm_fleet*": C.c_void_p, "const uint8_t*": _u8p, "const double*": _dp, "double*": _dp, "const uint64_t*": _u64p,
             "uint32_t*": _u32p, "int*": C.POINTER(C.c_int), "double": C.c_double, "uint32_t": C.c_uint32, "int": C.c_int}
    for name in ("cssm_fleet_smooth", "cssm_fleet_smooth_last_ms"):
        assert name in sig and hasattr(lib, name)
        m = re.search(r"\bint " + name + r"\(([^)]*)\);", header)
        assert m, f"{name} is not declared in include/cssm_pf.h"
        args = [" ".join(a.split()[:-1]) for a in m.group(1).replace("\n", " ").split(",")]
        assert [ctype[a] for a in args] == list(sig[name][2]), (name, args)
        assert sig[name][1] is C.c_int
    assert _abi.CSSM_OPT_SMOOTH_STAGING == int(re.search(r"#define CSSM_OPT_SMOOTH_STAGING (\d+)", header).group(1)) == 14


def _call(lib, off=(0, 2), interval=0.975, flags=0, n_traj=4, null=()):
    off = np.asarray(off, dtype=np.uint64)
    t = np.arange(4.0); y = np.ones(4); ll = np.zeros(1); rc = np.zeros(1, dtype=np.int32)
    p = lambda a, ty: None if a is None else a.ctypes.data_as(ty)
    g = lambda name, a: None if name in null else a
    return lib.cssm_fleet_smooth(None, p(g("off", off), _u64p), p(g("t", t), _dp), p(g("y", y), _dp), None, n_traj, interval, flags,
                                 p(g("ll", ll), _dp), *([None] * 6), None, p(g("rc", rc), C.POINTER(C.c_int)))


def test_whole_call_refusals_are_made_before_the_fleet_is_looked_at_in_interpolates_order():
    lib = load_library()
    # every earlier refusal wins over every later one: each call also carries all the later faults
    later = {"flags": _abi.CSSM_INTERP_REFERENCE_PAIRING, "n_traj": 0}
    for kw, word in (({"null": ("off", "ll", "t"), "off": (1, 2), "interval": 2.0}, b"off is null"),
                     ({"null": ("ll", "t"), "off": (1, 2), "interval": 2.0}, b"ll_out / rc_out is null"),
                     ({"null": ("rc", "t"), "off": (1, 2), "interval": 2.0}, b"ll_out / rc_out is null"),
                     ({"null": ("t",), "off": (1, 2), "interval": 2.0}, b"off[0] must be 0"),
                     ({"null": ("y",), "interval": 2.0}, b"null data"),
                     ({"interval": 0.0}, b"interval must be in (0, 1]")):
        assert _call(lib, **{**later, **kw}) == A, kw
        assert word in lib.cssm_last_error(), (kw, lib.cssm_last_error())
    assert _call(lib, flags=_abi.CSSM_INTERP_REFERENCE_PAIRING, n_traj=0) == A
    assert b"cssm_fleet_smooth" in lib.cssm_last_error() and b"CSSM_INTERP_REFERENCE_PAIRING is not offered" in lib.cssm_last_error()
    assert _call(lib, flags=3) == A and b"CSSM_INTERP_REFERENCE_PAIRING is not offered" in lib.cssm_last_error()
    assert _call(lib, flags=6, n_traj=0) == A and b"unknown flag bits 0x6" in lib.cssm_last_error()
    for bad in (0, _abi.FLEET_MAX_N + 1, 2**32 - 1):
        assert _call(lib, n_traj=bad) == A
        assert b"n_traj must be in [1, CSSM_FLEET_MAX_N = 4096]" in lib.cssm_last_error() and str(bad).encode() in lib.cssm_last_error()
    assert _call(lib, n_traj=_abi.FLEET_MAX_N) == A and b"null fleet" in lib.cssm_last_error()
    assert _call(lib) == A and b"null fleet" in lib.cssm_last_error()


def test_last_ms_without_a_fleet_leaves_the_array_alone():
    lib = load_library()
    ms = np.full(3, 7.0)
    assert lib.cssm_fleet_smooth_last_ms(None, ms.ctypes.data_as(_dp)) == A and list(ms) == [7.0, 7.0, 7.0]
    assert b"null" in lib.cssm_last_error()


# 5 ------------------------------------------------------------------------------------------------------------------------------
class _Recorder:
    """stands where the library stands: keeps what cssm_fleet_smooth was handed and fills the outputs with recognisable values"""

    def __init__(self, S, d):
        self.S, self.d, self.calls = S, d, []

    def cssm_fleet_smooth(self, h, off, t, y, has, n_traj, interval, flags, ll, sm, slo, sup, em, elo, eup, traj, rc):
        o = np.ctypeslib.as_array(off, (self.S + 1,)).copy()
        R = int(o[-1])
        rows = R + self.S
        self.calls.append({"off": o, "t": np.ctypeslib.as_array(t, (max(R, 1),)).copy(), "has": np.ctypeslib.as_array(has, (max(R, 1),)).copy(),
                           "n_traj": n_traj, "interval": interval, "flags": flags, "traj": traj is not None})
        np.ctypeslib.as_array(ll, (self.S,))[:] = np.arange(self.S) + 0.5
        np.ctypeslib.as_array(sm, (rows, self.d))[:] = np.arange(rows * self.d).reshape(rows, self.d)
        np.ctypeslib.as_array(elo, (rows,))[:] = np.arange(rows) + 0.25
        if traj is not None:
            np.ctypeslib.as_array(traj, (rows, n_traj))[:] = np.arange(rows * n_traj).reshape(rows, n_traj)
        return 0


def _handleless(S=3, n=10, d=2):
    fl = NativePfFleet.__new__(NativePfFleet)
    fl.S, fl.n, fl.d, fl.generation, fl._h, fl.seeds = S, n, d, 0, C.c_void_p(), [0] * S
    fl.lib = _Recorder(S, d)
    return fl


DATAS = [(np.arange(3.0), np.ones(3), None), (np.zeros(0), np.zeros(0), None), (np.array([5.0, 6.0]), np.array([2.0, 1.0]), np.array([0, 1]))]


@pytest.mark.parametrize("want", [False, True])
def test_what_smooth_hands_over_and_how_it_splits_the_rows(want):
    fl = _handleless()
    out = fl.smooth(DATAS, n_traj=None, interval=0.9, want_trajectories=want)
    call = fl.lib.calls[0]
    assert list(call["off"]) == [0, 3, 3, 5] and list(call["t"]) == [0, 1, 2, 5, 6] and list(call["has"]) == [1, 1, 1, 0, 1]
    assert (call["n_traj"], call["interval"], call["flags"], call["traj"]) == (10, 0.9, 0, want)       # None: as many as particles
    assert len(out) == (4 if want else 3)
    ll, rows, rc = out[:3]
    assert list(ll) == [0.5, 1.5, 2.5] and not rc.any() and len(rows) == 3
    first = [0, 4, 5]                                          # off[k] + k
    for k, T in enumerate((3, 0, 2)):
        assert rows[k][0].shape == (T + 1, 2) and rows[k][4].shape == (T + 1,)
        np.testing.assert_array_equal(rows[k][0], np.arange(16).reshape(8, 2)[first[k]:first[k] + T + 1])
        np.testing.assert_array_equal(rows[k][4], np.arange(8)[first[k]:first[k] + T + 1] + 0.25)
        if want:
            assert out[3][k].dtype == np.uint32 and out[3][k].shape == (T + 1, 10)
            np.testing.assert_array_equal(out[3][k], np.arange(80).reshape(8, 10)[first[k]:first[k] + T + 1])
    fl.smooth(DATAS, n_traj=7)
    assert fl.lib.calls[1]["n_traj"] == 7 and fl.lib.calls[1]["interval"] == 0.975


def test_what_smooth_refuses_before_any_device_call():
    fl = _handleless()
    with pytest.raises(ValueError, match="per series"):
        fl.smooth(DATAS[:2])
    for bad in (0, -1, _abi.FLEET_MAX_N + 1):
        with pytest.raises(ValueError, match="n_traj must be in"):
            fl.smooth(DATAS, n_traj=bad)
    off, t, y, has = NativePfFleet.pack(DATAS[:2], allow_empty=True)
    with pytest.raises(ValueError, match="S \\+ 1 = 4"):
        fl.smooth_packed(off, t, y, has)
    assert fl.lib.calls == []


def test_filter_fleet_smooth_returns_what_interpolate_returns():
    data = [Data(3.0, 1.0), Data(4.0, None), Data(5.0, 4.0)]
    rng = np.random.default_rng(7)
    arrays = tuple(rng.normal(size=(4, 2)) for _ in range(3)) + tuple(rng.normal(size=4) for _ in range(3))
    seen = []

    class Fleet:
        def smooth(self, split, n_traj, interval):
            seen.append(("smooth", n_traj, interval, [list(s[0]) for s in split]))
            return np.array([-2.5]), [arrays], np.zeros(1, dtype=np.int32)

        def interpolate(self, split, interval, reference_pairing):
            return np.array([-2.5]), [arrays], np.zeros(1, dtype=np.int32)

    ff = FilterFleet.__new__(FilterFleet)
    ff._fleet, ff.S = Fleet(), 1
    (ll, outs), = ff.smooth([data], n_traj=50, interval=0.9)
    (ll2, outs2), = ff.interpolate([data], 0.9)
    assert seen == [("smooth", 50, 0.9, [[3.0, 4.0, 5.0]])] and ll == ll2 == -2.5 and len(outs) == len(outs2) == 4
    for a, b in zip(outs, outs2):
        assert type(a) is type(b) and (a.time, a.observation, a.eta, a.etaIntervals, a.stateIntervals) == (b.time, b.observation, b.eta, b.etaIntervals,
                                                                                                          b.stateIntervals)
        np.testing.assert_array_equal(a.state, b.state)
    assert [o.observation for o in outs] == [None, 1.0, None, 4.0]


# 6 ------------------------------------------------------------------------------------------------------------------------------
# The long series of tests/test_gpu_fleet_smooth_truth.py: the "linear" model on cases.gaussian_series(100), no observation removed,
# N = 1000 particles, LONG_R replicates keyed LONG_SEED0 + r.  The truth is `rts` (closed form, no error bound).
LONG_N, LONG_T, LONG_R, LONG_SEED0 = 1000, 100, 128, 9000


def long_case():
    t, y, has = cases.gaussian_series(LONG_T)
    return cases.linear_model(), t, y, has


def rank_truth(model, t, y, has, M, interval=0.975):
    """test_grid_smoother.gaussian_truth with the quantiles taken at the probabilities the returned order statistics estimate: the
    0-based rank r of M values sits at (r + 1) / (M + 1) (the mean of its Beta law), and sel_ranks takes r = M - idx - 1 / idx - 1 for a
    state row and M - idx / idx for eta, idx = floor(interval M), clamped into the cloud.  At M = 1000 that is 2.498 % / 97.403 % for a
    state instead of 2.5 % / 97.5 %: 0.017 posterior standard deviations on the upper side, which R = 128 replicates of 1000 values
    resolve (their standard error is 0.0075)."""
    import grid_reference as gr
    import test_grid_smoother as tg
    from scipy.special import ndtri
    idx = int(np.floor(interval * M))
    clamp = lambda r: min(max(r, 0), M - 1)
    p = lambda r: (clamp(r) + 1.0) / (M + 1.0)
    tr = tg.gaussian_truth(model, t, y, has)
    spec = gr.spec_of(model)
    ms, Ps = gr.rts(spec, t, y, has)
    sd = np.sqrt(np.einsum("sii->si", Ps))
    gm = np.array([gr.gamma_moments(spec, ms[k], Ps[k], time) for k, time in enumerate(tg.row_times(t))])
    tr.lo, tr.hi = ms + ndtri(p(M - idx - 1)) * sd, ms + ndtri(p(idx - 1)) * sd
    tr.eta_lo, tr.eta_hi = gm[:, 0] + ndtri(p(M - idx)) * gm[:, 1], gm[:, 0] + ndtri(p(idx)) * gm[:, 1]
    return tr


def test_the_premise_genealogical_interpolation_is_rejected_on_the_long_series():
    """oracle.interpolate at N = 1000, T = 100: after a hundred resamplings the lineages that survive pass through few ancestors, the
    early rows' order statistics are too narrow, and z = (replicate mean - truth) / sqrt(s^2 / R) over the 101 rows is REJECTED by the
    criteria of tests/test_grid_smoother.py (rms <= 3 and max <= 8) on lower and upper.  R was chosen for that: at R = 32 lower / upper
    read rms 2.36 / 2.32 (max 6.7 / 6.1) and at R = 64 3.08 / 2.94 (max 7.6 / 7.2), both still accepted on one side; at R = 128 the rms
    is 4.06 / 3.94 and the max 9.2 / 9.0 against the 2.5 % / 97.5 % quantiles, and 4.07 / 3.62 with max 9.2 / 8.6 against the quantiles at
    the ranks' own probabilities (rank_truth), which this test and the GPU test use.  The means stay accepted (rms 1.08): what coalesces
    is the spread, not the location."""
    import test_grid_smoother as tg
    model, t, y, has = long_case()
    tr = rank_truth(model, t, y, has, LONG_N)
    o = oracle.OraclePf(model.descriptor(), LONG_N, 1)
    outs = []
    for r in range(LONG_R):
        o.reseed(LONG_SEED0 + r)
        outs.append(o.interpolate(t, y, has))
    runs = tg.stack(outs)
    for name, x, ref, reject in (("mean", runs[0], tr.mean, False), ("lower", runs[1], tr.lo, True), ("upper", runs[2], tr.hi, True)):
        rms, mx, at = tg.zscore(x, ref, np.zeros_like(ref))
        print(f"    oracle interpolate {name:5}: z rms {np.round(rms, 2).tolist()}  max {np.round(mx, 2).tolist()} at row {at.tolist()}")
        assert tg.accepted(rms, mx) == (not reject), (name, rms, mx)


# 7 ------------------------------------------------------------------------------------------------------------------------------
def test_both_kernels_are_instantiated_per_dimension_and_tested_over_all_sixteen():
    """tests/test_fleet_matrix_host.py keeps such a list for the kernels that were there before this file; the smoother's two kernels are
    launched through a function template per kernel and are held to the same rule here: every kernel cssm_fleet_smooth.hip defines is
    dispatched over the latent dimension, and one GPU test runs cases.dim_model(d) for d = 1 .. 16 through the call."""
    import importlib
    import inspect
    src = open(os.path.join(ROOT, "composablestatespacemodels_amd", "csrc", "cssm_fleet_smooth.hip")).read()
    defined = set(re.findall(r"__global__[^;{]*?void\s+(k_fleet_\w+)\(", src))
    assert defined == {"k_fleet_backsim", "k_fleet_smooth_rows"}
    launched = set(re.findall(r"hipLaunchKernelGGL\(\(?(k_fleet_\w+)<D", src))
    assert launched == defined and len(re.findall(r"DISPATCH_D\(", src)) == 3
    mod = importlib.import_module("test_gpu_fleet_smooth")
    fn = mod.test_every_latent_dimension
    marks = [m for m in fn.pytestmark if m.name == "parametrize" and m.args[0] == "d"]
    assert marks and list(marks[0].args[1]) == list(range(1, 17))
    body = inspect.getsource(fn)
    assert "cases.dim_model(d)" in body and ".smooth(" in body
    assert any(m.name == "gpu" for m in (mod.pytestmark if isinstance(mod.pytestmark, list) else [mod.pytestmark]))
