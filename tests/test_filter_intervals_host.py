"""CPU-only checks of the single handle's filtered intervals (include/cssm_pf.h: cssm_pf_filter_intervals, cssm_pf_filter_intervals_more,
cssm_pf_step_intervals, cssm_pf_intervals_last_ms):

  * the sequential twin of the two-rank selection (tests/cpp/intervals_twin.c, written on the arithmetic the kernels share with the
    host: composablestatespacemodels_amd/csrc/cssm_intervals.hip.h) against a sort of the order keys, on the clouds that break a
    selection and on seeded random multisets with heavy ties; its passes never exceed the enqueued number, its candidates at the finish
    never the cap; the counted budget of a row (launches, reads of the keys);
  * the bindings against the header and the refusals made before the GPU is looked at;
  * what NativePf and Filter hand to the calls and make of the rows, against a recording stub.

The helpers that build the twin and the crafted clouds are imported by tests/test_gpu_filter_intervals.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cases
from composablestatespacemodels_amd import Data, _abi, load_library
from composablestatespacemodels_amd.filter import (CredibleInterval, Filter, FilterInit, NativePf, ParticleFilter, PfOut, Resampling,
                                                   pfouts_from_rows)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_dp, _u64p = C.POINTER(C.c_double), C.POINTER(C.c_uint64)
_TWIN = None
INTERVALS = (0.975, 0.5, 1.0, 1e-9)     # 1.0: ranks 0 and N - 1; 1e-9: floor(interval N) = 0, the ranks clamp
SIZES = (64, 4097, 70001)


def build_intervals_twin(out_dir=None) -> C.CDLL:
    """tests/cpp/intervals_twin.c built with the gcc line of the other twins (once per process)."""
    global _TWIN
    if _TWIN is None:
        import tempfile
        so = os.path.join(str(out_dir or tempfile.mkdtemp(prefix="intervals_twin_")), "intervals_twin.so")
        subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-mfma", "-std=c99", "-shared", "-fPIC", "-o", so,
                               os.path.join(ROOT, "tests", "cpp", "intervals_twin.c"), "-lm"])
        lib = C.CDLL(so)
        lib.twin_iv_select.argtypes = [_dp, C.c_uint64, C.c_uint64, C.c_uint64, _dp, _u64p]
        lib.twin_iv_select.restype = C.c_int
        lib.twin_iv_ranks.argtypes = [C.c_uint64, C.c_double, C.c_int, _u64p]
        lib.twin_iv_ranks.restype = None
        lib.twin_iv_constants.argtypes = [C.c_uint64, _u64p]
        lib.twin_iv_constants.restype = None
        _TWIN = lib
    return _TWIN


def order_keys(x) -> np.ndarray:
    """cssm_order_key of every element: unsigned, ascending with the double, -0.0 below +0.0."""
    u = np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)
    return np.where(u >> np.uint64(63), ~u, u | np.uint64(1 << 63))


def ranks(n: int, interval: float, state_row: bool):
    """sel_ranks' rule (composablestatespacemodels_amd/csrc/cssm_kernels.hip.h), restated: getCredibleInterval takes the sorted elements
    (n - index - 1, index - 1) for a state row, getOrderStatistic (n - index, index) for eta, index = floor(interval n); clamped into
    the cloud."""
    idx = int(np.floor(interval * n))
    lo, hi = (n - idx - 1, idx - 1) if state_row else (n - idx, idx)
    return min(max(lo, 0), n - 1), min(max(hi, 0), n - 1)


def exact_order_statistics(x, interval: float, state_row: bool):
    """The two order statistics of x by a full sort of the order keys: (lower, upper) as doubles with the selected elements' bits."""
    k = np.sort(order_keys(x))
    lo, hi = ranks(len(k), interval, state_row)
    sel = np.array([k[lo], k[hi]], dtype=np.uint64)
    return np.where(sel >> np.uint64(63), sel & np.uint64((1 << 63) - 1), ~sel).view(np.float64)


def twin_select(x, interval: float, state_row: bool = True):
    """(the two order statistics, stats[8]) of the twin on the row x (the stats: tests/cpp/intervals_twin.c)."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    tw = build_intervals_twin()
    r = (C.c_uint64 * 2)()
    tw.twin_iv_ranks(len(x), float(interval), 1 if state_row else 0, r)
    assert (r[0], r[1]) == ranks(len(x), interval, state_row)
    out, stats = np.zeros(2), (C.c_uint64 * 8)()
    rc = tw.twin_iv_select(x.ctypes.data_as(_dp), len(x), r[0], r[1], out.ctypes.data_as(_dp), stats)
    assert rc == 0, (rc, list(stats))
    return out, list(stats)


def twin_constants(n: int):
    """(bins, cap, enqueued passes, candidate slots of a row of n)."""
    c = (C.c_uint64 * 4)()
    build_intervals_twin().twin_iv_constants(n, c)
    return tuple(int(v) for v in c)


def crafted_clouds(n: int, interval: float):
    """The clouds that break a selection, by name: rows of n doubles."""
    rng = np.random.default_rng(cases.SEED + n)
    out = {"all equal": np.full(n, 1.25)}
    a = np.full(n, -0.75); a[n // 3] = -1e9
    out["one outlier below"] = a
    a = np.full(n, -0.75); a[n // 3] = 1e9
    out["one outlier above"] = a
    rl, ru = ranks(n, interval, True)
    for name, r in (("lower", rl), ("lower + 1", rl + 1), ("upper", ru), ("upper + 1", ru + 1)):
        r = min(max(r, 1), n - 1)
        a = np.where(np.arange(n) < r, 2.0, 3.0)
        out[f"two values split at {name}"] = rng.permutation(a)
    out["shared top 40 bits"] = rng.permutation(1.0 + np.arange(n) * 2.0 ** -50)
    out["zeros and subnormals"] = rng.choice(np.array([-0.0, 0.0, 5e-324, -5e-324, 1e-310, -1e-310, 2.2e-308]), size=n)
    lad = 10.0 ** np.linspace(-300.0, 300.0, n)
    out["sign-mixed ladder"] = rng.permutation(np.where(np.arange(n) % 2 == 0, lad, -lad))
    a = rng.standard_normal(n); a[::7] = np.inf; a[3::11] = -np.inf
    out["infinities"] = a
    multi = np.sort(rng.integers(-3, 4, size=n).astype(np.float64) * 0.5 + rng.choice([0.0, 2.0 ** -40], size=n))
    out["multiset ascending"] = multi
    out["multiset descending"] = multi[::-1].copy()
    out["multiset shuffled"] = rng.permutation(multi)
    return out


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("interval", INTERVALS)
def test_twin_selects_the_exact_order_statistics_of_the_crafted_clouds(n, interval):
    bins, cap, rounds, _ = twin_constants(n)
    rows = {}
    for name, x in crafted_clouds(n, interval).items():
        for state_row in (True, False):
            got, st = twin_select(x, interval, state_row)
            np.testing.assert_array_equal(_bits(got), _bits(exact_order_statistics(x, interval, state_row)), err_msg=f"{name} state_row={state_row}")
            assert st[0] <= rounds and st[1] <= st[0], (name, st)
            assert st[2] <= cap and st[3] <= cap, (name, st)
        rows[name] = _bits(twin_select(x, interval)[0])
    np.testing.assert_array_equal(rows["multiset ascending"], rows["multiset descending"])
    np.testing.assert_array_equal(rows["multiset ascending"], rows["multiset shuffled"])


def test_twin_on_random_multisets_with_heavy_ties():
    rng = np.random.default_rng(cases.SEED)
    for it in range(200):
        n = int(rng.choice([1, 2, 3, 63, 64, 65, 1000, 4096, 4097, 20001])) if it % 20 else 70001
        kind = it % 5
        if kind == 0:
            x = rng.integers(0, 1 + it % 7, size=n).astype(np.float64)
        elif kind == 1:
            x = rng.choice(rng.standard_normal(1 + it % 50), size=n)                       # a resampled cloud: few distinct particles
        elif kind == 2:
            x = np.where(rng.random(n) < 0.6, 1.0, 1.0 + rng.integers(0, 3, size=n) * 2.0 ** -52)
        elif kind == 3:
            x = np.concatenate([np.full(n - n // 4, 3.0), rng.standard_normal(n // 4) * 1e-300])
        else:
            x = np.exp(rng.standard_normal(n)) * rng.choice([1.0, -1.0, 0.0], size=n)
        _, cap, rounds, _ = twin_constants(n)
        for interval in INTERVALS:
            got, st = twin_select(x, interval, bool(it & 1))
            np.testing.assert_array_equal(_bits(got), _bits(exact_order_statistics(x, interval, bool(it & 1))), err_msg=f"it={it} n={n} interval={interval}")
            assert st[0] <= rounds and st[2] <= cap and st[3] <= cap, (it, n, st)


def test_counted_budget_of_a_row():
    """At most 8 launches per row (the fill, the enqueued passes, the finish) and, in the ordinary case -- a cloud of distinct values of
    one sign, or spread round zero --, the cloud read once and its keys twice: 3 reads, against 9 of cssm_pf_summary."""
    n = 70001
    _, _, rounds, cand_max = twin_constants(n)
    assert 1 + rounds + 1 <= 8
    assert cand_max == max(4096, n // 4)
    rng = np.random.default_rng(cases.SEED)
    for x in (np.exp(rng.standard_normal(n)), rng.standard_normal(n), 5.0 + 0.01 * rng.standard_normal(n)):
        for interval in (0.975, 0.5):
            _, st = twin_select(x, interval)
            assert 1 + st[1] <= 3, st
    # all-equal clouds finish without a pass
    assert twin_select(np.full(n, 2.0), 0.975)[1][0] == 0


def test_bindings_and_refusals_before_the_gpu():
    lib = load_library()
    bound = {s[0]: s for s in _abi.SYMBOLS}
    for name in ("cssm_pf_filter_intervals", "cssm_pf_filter_intervals_more", "cssm_pf_step_intervals", "cssm_pf_intervals_last_ms"):
        assert name in bound and hasattr(lib, name), name
    assert len(bound["cssm_pf_filter_intervals"][2]) == 15 and bound["cssm_pf_filter_intervals"][2] == bound["cssm_pf_filter_intervals_more"][2]
    assert len(bound["cssm_pf_step_intervals"][2]) == 13
    t = np.zeros(2); six = [None] * 6
    A = _abi.CSSM_EINVAL_ARG
    assert lib.cssm_pf_filter_intervals(None, t.ctypes.data_as(_dp), t.ctypes.data_as(_dp), None, 2, 0.975, None, None, None, *six) == A
    assert b"null argument" in lib.cssm_last_error()
    assert lib.cssm_pf_filter_intervals_more(None, t.ctypes.data_as(_dp), t.ctypes.data_as(_dp), None, 2, 0.975, None, None, None, *six) == A
    assert lib.cssm_pf_step_intervals(None, 0.0, 0.0, 1, 0.975, None, None, *six) == A
    assert b"null handle" in lib.cssm_last_error()
    ms = np.full(2, 7.0)
    assert lib.cssm_pf_intervals_last_ms(None, ms.ctypes.data_as(_dp)) == A and list(ms) == [7.0, 7.0]


# ---- the Python surface against a recording stub ---------------------------------------------------------------------------------------
D_STUB, N_STUB = 3, 11


class StubLib:
    """``NativePf.lib``: the three calls check their argument count against ``_abi.SYMBOLS``, record their inputs and fill output j with
    1000 (j + 1) + index through the pointers they were given."""

    def __init__(self):
        self.calls = []
        self.sig = {s[0]: s[2] for s in _abi.SYMBOLS}

    @staticmethod
    def _fill(ptr, count, j):
        if ptr is not None:
            np.ctypeslib.as_array(ptr, shape=(count,))[:] = 1000.0 * (j + 1) + np.arange(count)

    def _batch(self, name, extra, h, t, y, has, T, interval, ll, ll_t, ess_t, *six):
        assert 9 + len(six) == len(self.sig[name]) and len(six) == 6
        rec = {"name": name, "T": T, "interval": interval, "t": np.ctypeslib.as_array(t, shape=(T,)).copy(), "y": np.ctypeslib.as_array(y, shape=(T,)).copy(),
               "has": None if has is None else np.ctypeslib.as_array(has, shape=(T,)).copy()}
        self.calls.append(rec)
        ll._obj.value = 42.5
        np.ctypeslib.as_array(ll_t, shape=(T,))[:] = 10.0 + np.arange(T)
        np.ctypeslib.as_array(ess_t, shape=(T,))[:] = 20 + np.arange(T)
        R = T + extra
        for j, p in enumerate(six):
            self._fill(p, R * D_STUB if j < 3 else R, j)
        return 0

    def cssm_pf_filter_intervals(self, *a):
        return self._batch("cssm_pf_filter_intervals", 1, *a)

    def cssm_pf_filter_intervals_more(self, *a):
        return self._batch("cssm_pf_filter_intervals_more", 0, *a)

    def cssm_pf_step_intervals(self, h, t, y, has, interval, ll, ess, m, lo, hi, em, el, eu):
        assert len(self.sig["cssm_pf_step_intervals"]) == 13
        self.calls.append({"name": "cssm_pf_step_intervals", "t": t, "y": y, "has": has, "interval": interval})
        ll._obj.value, ess._obj.value = -3.5, 9
        for j, p in enumerate((m, lo, hi)):
            self._fill(p, D_STUB, j)
        em._obj.value, el._obj.value, eu._obj.value = 4000.0, 5000.0, 6000.0
        return 0

    def cssm_pf_summary(self, h, interval, m, lo, hi, em, el, eu):
        self.calls.append({"name": "cssm_pf_summary", "interval": interval})
        for j, p in enumerate((m, lo, hi)):
            np.ctypeslib.as_array(p, shape=(D_STUB,))[:] = -1000.0 * (j + 1) - np.arange(D_STUB)
        em._obj.value, el._obj.value, eu._obj.value = -4000.0, -5000.0, -6000.0
        return 0

    def cssm_pf_init_from(self, h, t0, state):
        self.calls.append({"name": "cssm_pf_init_from", "t0": t0})
        return 0

    def cssm_pf_intervals_last_ms(self, h, ms):
        np.ctypeslib.as_array(ms, shape=(2,))[:] = (3.0, 2.0)
        return 0


def stub_pf() -> NativePf:
    pf = object.__new__(NativePf)
    pf.lib, pf._h, pf.n, pf.d, pf.generation = StubLib(), None, N_STUB, D_STUB, 0
    return pf


def _stub_filter(cls, *extra):
    flt = cls(cases.c2_model(), Resampling.systematicResampling, *extra)
    flt._pf = stub_pf()
    flt._ensure = lambda n: flt._pf
    return flt


def test_native_pf_marshals_the_three_calls():
    pf = stub_pf()
    t, y, has = np.array([0.0, 1.0, 1.0, 2.5]), np.array([1.0, 0.0, 3.0, 2.0]), np.array([1, 0, 1, 1], dtype=np.uint8)
    ll, ll_t, ess_t, m, lo, hi, em, el, eu = pf.filter_intervals(t, y, has, interval=0.9)
    c = pf.lib.calls[-1]
    assert c["name"] == "cssm_pf_filter_intervals" and c["T"] == 4 and c["interval"] == 0.9 and pf.generation == 1
    np.testing.assert_array_equal(c["t"], t); np.testing.assert_array_equal(c["y"], y); np.testing.assert_array_equal(c["has"], has)
    assert ll == 42.5 and list(ll_t) == [10.0, 11.0, 12.0, 13.0] and list(ess_t) == [20, 21, 22, 23] and ess_t.dtype == np.int32
    assert m.shape == lo.shape == hi.shape == (5, D_STUB) and em.shape == el.shape == eu.shape == (5,)
    for j, a in enumerate((m, lo, hi, em, el, eu)):
        np.testing.assert_array_equal(a.ravel(), 1000.0 * (j + 1) + np.arange(a.size))
    r = pf.filter_intervals_more(t, y)
    assert pf.lib.calls[-1]["name"] == "cssm_pf_filter_intervals_more" and pf.lib.calls[-1]["has"] is None and pf.lib.calls[-1]["interval"] == 0.975
    assert r[3].shape == (4, D_STUB) and r[6].shape == (4,) and pf.generation == 2
    ll, ess, m, lo, hi, em, el, eu = pf.step_intervals(3.0, None)
    c = pf.lib.calls[-1]
    assert (c["t"], c["y"], c["has"], c["interval"]) == (3.0, 0.0, 0, 0.975) and pf.generation == 3
    assert (ll, ess, em, el, eu) == (-3.5, 9, 4000.0, 5000.0, 6000.0) and list(lo) == [2000.0, 2001.0, 2002.0]
    assert pf.step_intervals(3.0, 2.0, interval=0.5)[1] == 9 and pf.lib.calls[-1]["has"] == 1 and pf.lib.calls[-1]["y"] == 2.0
    assert pf.intervals_last_ms() == (3.0, 2.0)


def _expect(time, obs, r, shift=0.0, sign=1.0):
    return PfOut(time, obs, sign * (4000.0 + r) , CredibleInterval(sign * (5000.0 + r), sign * (6000.0 + r)),
                 sign * (1000.0 + D_STUB * r + np.arange(D_STUB)),
                 [CredibleInterval(sign * (2000.0 + D_STUB * r + k), sign * (3000.0 + D_STUB * r + k)) for k in range(D_STUB)])


def _same_pfout(a: PfOut, b: PfOut):
    assert (a.time, a.observation, a.eta, a.etaIntervals, a.stateIntervals) == (b.time, b.observation, b.eta, b.etaIntervals, b.stateIntervals)
    np.testing.assert_array_equal(a.state, b.state)


def test_filter_intervals_assembles_pfouts_from_the_rows():
    flt = _stub_filter(Filter)
    data = [Data(2.0, 1.0), Data(0.5, None), Data(3.0, 4.0)]
    ll, outs = flt.filterIntervals(data, N_STUB, interval=0.8)
    c = flt._pf.lib.calls[-1]
    assert c["name"] == "cssm_pf_filter_intervals" and c["interval"] == 0.8 and list(c["has"]) == [1, 0, 1] and list(c["t"]) == [2.0, 0.5, 3.0]
    assert ll == 42.5 and len(outs) == 4
    for r, (tt, ob) in enumerate([(0.5, None), (2.0, 1.0), (0.5, None), (3.0, 4.0)]):      # the first: the initial cloud at min t, no observation
        _same_pfout(outs[r], _expect(tt, ob, r))
    # stepIntervals: the state and its PfOut from one call
    st0 = flt._state(3.0, 4.0, ll, 5)
    st, out = flt.stepIntervals(st0, Data(4.0, 2.0))
    assert (st.t, st.observation, st.ll, st.ess) == (4.0, 2.0, -3.5, 9) and st._generation == flt._pf.generation
    _same_pfout(out, _expect(4.0, 2.0, 0))
    with pytest.raises(RuntimeError):
        flt.stepIntervals(st0, Data(5.0, 1.0))                                            # not the current state any more
    with pytest.raises(ValueError):
        pfouts_from_rows([0.0], [None, 1.0], tuple(np.zeros((1, 3)) for _ in range(3)) + tuple(np.zeros(1) for _ in range(3)))


def test_filter_init_puts_the_given_state_s_summary_in_front():
    flt = _stub_filter(FilterInit, [0.0, 0.1, 0.2])
    data = [Data(1.0, 1.0), Data(2.0, 0.0)]
    ll, outs = flt.filterIntervals(data, N_STUB)
    names = [c["name"] for c in flt._pf.lib.calls]
    assert names == ["cssm_pf_init_from", "cssm_pf_summary", "cssm_pf_filter_intervals_more"]
    assert len(outs) == 3 and ll == 42.5
    _same_pfout(outs[0], PfOut(1.0, None, -4000.0, CredibleInterval(-5000.0, -6000.0), -1000.0 - np.arange(D_STUB),
                               [CredibleInterval(-2000.0 - k, -3000.0 - k) for k in range(D_STUB)]))
    _same_pfout(outs[1], _expect(1.0, 1.0, 0))
    _same_pfout(outs[2], _expect(2.0, 0.0, 1))


def test_get_intervals_is_a_summary_at_the_reference_s_interval():
    """What the batch rows are held to on the GPU: ParticleFilter.getIntervals = the handle's summary at 0.975."""
    flt = _stub_filter(Filter)
    out = ParticleFilter.getIntervals(flt.mod, flt._state(1.0, 2.0, 0.0, 3))
    assert flt._pf.lib.calls[-1] == {"name": "cssm_pf_summary", "interval": 0.975} and out.eta == -4000.0 and out.time == 1.0
