"""CPU-only checks of the fleet's `filter` and PMMH (include/cssm_pf.h: cssm_fleet_filter, cssm_fleet_pmmh_run): the ctypes view against
the header, the refusals that come before any device call, the no-device error, and -- on the oracle alone -- the premise of the GPU
PMMH test: every one of its chains both accepts and rejects."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import cases
import fleet_pmmh_cases as fc
from composablestatespacemodels_amd import CssmError, Data, _abi, load_library
from composablestatespacemodels_amd.filter import FilterFleet, NativePfFleet, Resampling
from composablestatespacemodels_amd.pmmh import pmmh_fleet_pack, pmmh_native_fleet
from test_fleet_host import _ctype_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("cssm_fleet_filter", "cssm_fleet_pmmh_run", "cssm_fleet_pmmh_last_split")


def _p(a, ty=C.c_double):
    return a.ctypes.data_as(C.POINTER(ty))


def test_ctypes_signatures_of_the_new_entry_points_match_the_header():
    src = open(os.path.join(ROOT, "include", "cssm_pf.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    decls = {d[1]: d for d in re.findall(r"^\s*([A-Za-z_][\w\s\*]*?)\b(cssm_fleet_\w+)\s*\(([^;]*?)\)\s*;", src, flags=re.M)}
    bound = {s[0]: s for s in _abi.SYMBOLS}
    lib = load_library()
    for name in NEW:
        assert name in decls and name in bound and hasattr(lib, name), name
        ret, _, args = decls[name]
        want = [_ctype_of(re.sub(r"\b\w+$", "", a.strip()) if not a.strip().endswith("*") else a) for a in args.split(",")]
        assert bound[name][1] == _ctype_of(ret) and list(bound[name][2]) == want, (name, bound[name][2], want)
    assert len(bound["cssm_fleet_filter"][2]) == 11 and len(bound["cssm_fleet_pmmh_run"][2]) == 15
    assert "Not here: `filter`'s sampled path" not in open(os.path.join(ROOT, "include", "cssm_pf.h")).read()


def test_filter_refusals_that_need_no_fleet_come_first():
    """cssm_fleet_filter with NO fleet: each refusal below is reported as itself, so it was made before the fleet (and any device) was
    looked at; only a call with nothing else to refuse reaches "null fleet"."""
    lib = load_library()
    off = np.array([0, 3], dtype=np.uint64); t = np.arange(3.0); y = np.ones(3)
    ll = np.zeros(1); rc = np.zeros(1, dtype=np.int32); last = np.zeros(3); path = np.zeros(12)

    def call(off_=off, t_=t, y_=y, ll_=ll, path_=path, last_=last, rc_=rc):
        q = lambda a, ty=C.c_double: None if a is None else _p(a, ty)
        r = lib.cssm_fleet_filter(None, q(off_, C.c_uint64), q(t_), q(y_), None, q(ll_), None, None, q(path_), q(last_), q(rc_, C.c_int))
        return r, lib.cssm_last_error()

    for kw, word in (({"off_": None}, b"off is null"), ({"rc_": None}, b"rc_out"), ({"ll_": None}, b"ll_out"), ({"t_": None}, b"null data"),
                     ({"y_": None}, b"null data"), ({"path_": None, "last_": None}, b"cssm_fleet_ll_filter"),
                     ({"off_": np.array([1, 3], dtype=np.uint64)}, b"off[0] must be 0"), ({}, b"null fleet"),
                     ({"path_": None}, b"null fleet"), ({"last_": None}, b"null fleet")):
        r, msg = call(**kw)
        assert r == _abi.CSSM_EINVAL_ARG and word in msg, (kw.keys(), msg)


def test_pmmh_refusals_that_need_no_fleet_come_first():
    lib = load_library()
    model = cases.c2_model()
    desc = model.descriptor()
    th = np.array(model.parameters().flattenParams())
    nt = th.size
    off = np.array([0, 3], dtype=np.uint64); t = np.arange(3.0); y = np.ones(3); sd = np.array([7], dtype=np.uint64)
    ll = np.zeros(2); tho = np.zeros((2, nt)); acc = np.zeros(2, dtype=np.int32); last = np.zeros((2, 3))

    def call(desc_=desc, th_=th, nt_=nt, off_=off, t_=t, sd_=sd, ll_=ll):
        q = lambda a, ty=C.c_double: None if a is None else _p(a, ty)
        r = lib.cssm_fleet_pmmh_run(None, desc_.ptr() if desc_ is not None else None, q(th_), nt_, 0.05, q(off_, C.c_uint64), q(t_), q(y), None,
                                    q(sd_, C.c_uint64), 2, q(ll_), q(tho), q(acc, C.c_int32), q(last))
        return r, lib.cssm_last_error()

    for kw in ({"desc_": None}, {"th_": None}, {"off_": None}, {"t_": None}, {"sd_": None}, {"ll_": None}):
        r, msg = call(**kw)
        assert r == _abi.CSSM_EINVAL_ARG and b"null" in msg, (kw.keys(), msg)
    r, msg = call(off_=np.array([2, 3], dtype=np.uint64))
    assert r == _abi.CSSM_EINVAL_ARG and b"off[0] must be 0" in msg
    for wrong in (nt - 1, nt + 1, 0):
        r, msg = call(nt_=wrong)
        assert r == _abi.CSSM_EINVAL_ARG and b"flattens to %d" % nt in msg, msg
    r, msg = call(desc_=cases.c4_model().descriptor(2))
    assert r == _abi.CSSM_EINVAL_DESC and b"LGCP" in msg and b"cssm_pmmh_run_batched" in msg
    r, msg = call()
    assert r == _abi.CSSM_EINVAL_ARG and b"null fleet" in msg


def _handleless(S, n=10, d=3):
    """a fleet object without a handle or a library: whatever touches the device through it raises AttributeError, not ValueError"""
    fl = NativePfFleet.__new__(NativePfFleet)
    fl.S, fl.n, fl.d, fl.generation, fl._h, fl.lib = S, n, d, 0, C.c_void_p(), None
    return fl


def test_python_refuses_bad_layouts_before_any_device_call():
    fl = _handleless(2)
    a = (np.zeros(2), np.zeros(2), None)
    with pytest.raises(ValueError, match="no records"):
        fl.filter([a, (np.zeros(0), np.zeros(0), None)])
    with pytest.raises(ValueError, match="one .* per series"):
        fl.filter([a])
    off, t, y, has = NativePfFleet.pack([a, a])
    for bad in (np.array([1, 2, 4], dtype=np.uint64), np.array([0, 3, 2], dtype=np.uint64), np.array([0, 2], dtype=np.uint64), off.astype(np.int64)):
        with pytest.raises(ValueError, match="off"):
            fl.filter_packed(bad, t, y, has)
    with pytest.raises(ValueError, match="t must be"):
        fl.filter_packed(off, t[:3], y, has)
    with pytest.raises(ValueError, match="t must be"):
        fl.filter_packed(off, None, y, has)
    with pytest.raises(ValueError, match="has must be"):
        fl.filter_packed(off, t, y, has.astype(np.float64))
    with pytest.raises(AttributeError):                       # (the premise: a layout that IS right goes on to the library)
        fl.filter_packed(off, t, y, has)


def test_pmmh_python_refuses_before_any_device_call():
    um, inits = cases.c2_unparam(), fc.chain_inits()[:2]
    data = fc.chain_data(0)
    with pytest.raises(ValueError, match="one seed per chain"):
        pmmh_native_fleet(um, inits, data, 100, 0.05, 3, [1])
    with pytest.raises(ValueError, match="one seed per chain"):
        pmmh_native_fleet(um, [], data, 100, 0.05, 3, [])
    with pytest.raises(ValueError, match="empty data set"):
        pmmh_native_fleet(um, inits, [], 100, 0.05, 3, [1, 2])
    with pytest.raises(ValueError, match="chain 1 has an empty data set"):
        pmmh_native_fleet(um, inits, [data, []], 100, 0.05, 3, [1, 2])
    with pytest.raises(ValueError, match="one per chain"):
        pmmh_native_fleet(um, inits, [data, data, data], 100, 0.05, 3, [1, 2])
    with pytest.raises(ValueError, match="same length"):
        pmmh_native_fleet(um, [inits[0], cases.c1_model().parameters()], data, 100, 0.05, 3, [1, 2])
    with pytest.raises(ValueError, match="holds 3 series"):
        pmmh_native_fleet(um, inits, data, 100, 0.05, 3, [1, 2], fleet=_handleless(3, 100))
    # one data set is every chain's; S data sets are laid out ragged, in order
    off, t, y, has = pmmh_fleet_pack(data, 3)
    T = len(data)
    assert list(off) == [0, T, 2 * T, 3 * T] and np.array_equal(t[:T], t[T:2 * T]) and np.array_equal(y[:T], y[2 * T:])
    off, t, y, has = pmmh_fleet_pack([fc.chain_data(0), fc.chain_data(1)], 2)
    t1, y1, h1 = fc.chain_arrays(1)
    assert list(off) == [0, 12, 27] and np.array_equal(t[12:], t1) and np.array_equal(y[12:], np.where(h1 != 0, y1, 0.0)) and np.array_equal(has[12:], h1)


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="this check is for hosts without a GPU")
def test_no_device_is_ehip_with_the_usual_message():
    um, inits = cases.c2_unparam(), fc.chain_inits()[:2]
    with pytest.raises(CssmError) as e:
        pmmh_native_fleet(um, inits, fc.chain_data(0), 100, 0.05, 3, [1, 2])
    assert e.value.code == _abi.CSSM_EHIP and "no CPU path" in str(e.value) and "cssm_pmmh_run_batched" not in str(e.value)
    with pytest.raises(CssmError) as e:
        with FilterFleet([cases.c2_model()] * 2, Resampling.systematicResampling, 100) as ff:
            ff.filter([fc.chain_data(0), fc.chain_data(1)])
    assert e.value.code == _abi.CSSM_EHIP and "no CPU path" in str(e.value)


@pytest.mark.parametrize("n", [100, 1000])
@pytest.mark.parametrize("delta", [0.01, 0.05, 0.25])
def test_premise_every_chain_of_the_gpu_test_accepts_and_rejects(n, delta):
    """The GPU test compares chains bit for bit; it says something about BOTH branches of the decision only if every chain takes both.
    On the oracle alone: 1 <= accepted[-1] <= 39 of 40 for each of the six chains (seen: 22-37 / 19-30 / 10-21 at delta 0.01 / 0.05 /
    0.25)."""
    got = []
    for k in range(fc.CHAINS):
        ll, th, acc, last = fc.oracle_chain(k, n, delta)
        got.append(int(acc[-1]))
        assert acc[0] == 1 and np.all(np.diff(acc) >= 0) and np.all(np.diff(acc) <= 1)
        assert np.all(np.isfinite(ll)) and np.all(np.isfinite(last))
    print(f"n = {n}, delta = {delta}: acceptances {got}")
    assert all(1 <= a <= fc.ITERS - 1 for a in got), got
