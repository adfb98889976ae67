"""-m gpu: PMMH on a fleet (cssm_fleet_pmmh_run): a Metropolis chain per series, every iteration's filters in one launch.  Chain k is
the oracle's pmmh and cssm_pmmh_run on a handle of its own, bit for bit -- ll, theta, the running acceptance count and the last sampled
state of every iteration -- and every chain compared takes both branches of the decision (test_fleet_pmmh_host.py shows it on the oracle
alone; asserted here again on the result)."""
import ctypes as C

import numpy as np
import pytest

import cases
import fleet_pmmh_cases as fc
from composablestatespacemodels_amd import CssmError, _abi
from composablestatespacemodels_amd.filter import FilterFleet, NativePfFleet, Resampling
from composablestatespacemodels_amd.pmmh import pmmh_fleet_pack, pmmh_native, pmmh_native_fleet, posterior_rows
from test_gpu_fleet import SEED, _perturbed

pytestmark = pytest.mark.gpu


class _Fixed:
    """an UnparamModel that builds one model whatever the parameters"""

    def __init__(self, model):
        self.model = model

    def run(self, p):
        return self.model


def assert_chain_equal(got, k, want):
    for a, b, name in zip(got, want, ("ll", "theta", "accepted", "last_state")):
        np.testing.assert_array_equal(a[k], b, err_msg=f"chain {k}: {name}")


@pytest.mark.parametrize("n", [100, 1000])
@pytest.mark.parametrize("delta", [0.05, 0.25])
def test_six_chains_on_data_of_their_own_equal_the_oracle_and_handles_of_their_own(n, delta):
    um, inits = cases.c2_unparam(), fc.chain_inits()
    datas = [fc.chain_data(k) for k in range(fc.CHAINS)]
    seeds = [fc.chain_seed(k) for k in range(fc.CHAINS)]
    got = pmmh_native_fleet(um, inits, datas, n, delta, fc.ITERS, seeds)
    assert got[0].shape == (6, 40) and got[1].shape[:2] == (6, 40) and got[2].shape == (6, 40) and got[3].shape == (6, 40, 3)
    for k in range(fc.CHAINS):
        assert_chain_equal(got, k, fc.oracle_chain(k, n, delta))
        assert_chain_equal(got, k, pmmh_native(um, inits[k], datas[k], n, delta, fc.ITERS, seed=seeds[k]))
        assert 1 <= got[2][k, -1] <= fc.ITERS - 1, (k, got[2][k])      # both branches of the decision were taken
        th, st = posterior_rows(got[1][k], got[3][k], burn_in=10, thin=3)
        np.testing.assert_array_equal(th, got[1][k][10::3])
        np.testing.assert_array_equal(st, got[3][k][10::3])


def test_one_data_set_shared_by_33_chains():
    um = cases.c2_unparam()
    S, n, iters = 33, 257, 10
    inits = [_perturbed(cases.c2_params, k) for k in range(S)]
    seeds = [SEED + 1000 + 3 * k for k in range(S)]
    data = fc.chain_data(1)
    got = pmmh_native_fleet(um, inits, data, n, 0.05, iters, seeds)
    for k in range(S):
        assert_chain_equal(got, k, pmmh_native(um, inits[k], data, n, 0.05, iters, seed=seeds[k]))
    assert len({tuple(r) for r in got[0]}) == S                          # the chains are not copies of one another


def test_one_iteration_and_a_fleet_reused_with_other_seeds():
    um, inits = cases.c2_unparam(), fc.chain_inits()
    S, n = fc.CHAINS, 300
    short = [fc.chain_data(k)[:6] for k in range(S)]                     # the second run needs larger buffers than the first
    long_ = [fc.chain_data(k) for k in range(S)]
    with NativePfFleet(um.run(inits[0]), n, S) as fl:
        for datas, iters, seeds in ((short, 1, [11 + k for k in range(S)]), (long_, 5, [901 + 7 * k for k in range(S)]),
                                    (short, 3, [11 + k for k in range(S)])):
            got = pmmh_native_fleet(um, inits, datas, n, 0.05, iters, seeds, fleet=fl)
            assert got[0].shape == (S, iters)
            for k in range(S):
                assert_chain_equal(got, k, pmmh_native(um, inits[k], datas[k], n, 0.05, iters, seed=seeds[k]))
            split, counted = fl.pmmh_last_split()
            assert counted == iters and all(v >= 0.0 for v in split)
        assert np.all(got[2][:, 0] == 1)                                 # from ll = -1e99 the first proposal is always accepted


def test_refusals_name_the_reason_and_leave_the_fleet_usable():
    um, inits = cases.c2_unparam(), fc.chain_inits()[:3]
    datas = [fc.chain_data(k) for k in range(3)]
    seeds = [5, 6, 7]
    n, iters = 100, 4

    def refused(code, words, fn):
        with pytest.raises(CssmError) as e:
            fn()
        assert e.value.code == code and all(w in str(e.value) for w in words), str(e.value)

    # an LGCP fleet, a cloud too large for a workgroup: refused where the fleet is made, naming the entry point that serves them
    c4 = cases.c4_model()
    refused(_abi.CSSM_EINVAL_DESC, ("LGCP", "cssm_pmmh_run_batched"),
            lambda: pmmh_native_fleet(_Fixed(c4), [c4.parameters()] * 2, datas[0], n, 0.05, iters, [1, 2]))
    refused(_abi.CSSM_EINVAL_ARG, ("particles", "cssm_pmmh_run_batched"),
            lambda: pmmh_native_fleet(um, inits, datas, _abi.FLEET_MAX_N + 1, 0.05, iters, seeds))
    # a resampler the fleet does not have
    refused(_abi.CSSM_EINVAL_ARG, ("systematic",), lambda: FilterFleet([um.run(p) for p in inits], Resampling.multinomialResampling, n))
    with NativePfFleet(um.run(inits[0]), n, 3) as fl:
        refused(_abi.CSSM_EINVAL_ARG, ("systematic",), lambda: fl.set_option(2, 1))
        # a descriptor of another structure in `desc` (C1, with its own parameter count: nothing else to refuse)
        c1 = cases.c1_model()
        th1 = np.ascontiguousarray([c1.parameters().flattenParams()] * 3, dtype=np.float64)
        off, t, y, has = pmmh_fleet_pack(datas, 3)
        sd = np.array(seeds, dtype=np.uint64)
        ll = np.zeros((3, iters)); th = np.zeros((3, iters, th1.shape[1])); acc = np.zeros((3, iters), dtype=np.int32); last = np.zeros((3, iters, 3))
        p = lambda a, ty=C.c_double: a.ctypes.data_as(C.POINTER(ty))
        rc = fl.lib.cssm_fleet_pmmh_run(fl._h, c1.descriptor().ptr(), p(th1), th1.shape[1], 0.05, p(off, C.c_uint64), p(t), p(y), p(has, C.c_uint8),
                                        p(sd, C.c_uint64), iters, p(ll), p(th), p(acc, C.c_int32), p(last))
        msg = fl.lib.cssm_last_error()
        assert rc == _abi.CSSM_EINVAL_DESC and b"structure" in msg and b"cssm_pmmh_run_batched" in msg, msg
        # an empty slice, a decreasing off: before the first iteration
        th0 = np.ascontiguousarray([q.flattenParams() for q in inits], dtype=np.float64)
        tho = np.zeros((3, iters, th0.shape[1]))
        desc = um.run(inits[0]).descriptor()
        for bad, word in ((np.array([0, 12, 12, 27], dtype=np.uint64), b"empty slice"), (np.array([0, 12, 8, 27], dtype=np.uint64), b"non-decreasing")):
            rc = fl.lib.cssm_fleet_pmmh_run(fl._h, desc.ptr(), p(th0), th0.shape[1], 0.05, p(bad, C.c_uint64), p(t), p(y), p(has, C.c_uint8),
                                            p(sd, C.c_uint64), iters, p(ll), p(tho), p(acc, C.c_int32), p(last))
            assert rc == _abi.CSSM_EINVAL_ARG and word in fl.lib.cssm_last_error()
        assert not ll.any() and not acc.any()                            # nothing ran
        # cssm_fleet_filter with neither output, on a real fleet
        rcs = np.zeros(3, dtype=np.int32)
        assert fl.lib.cssm_fleet_filter(fl._h, p(off, C.c_uint64), p(t), p(y), p(has, C.c_uint8), p(ll), None, None, None, None,
                                        p(rcs, C.c_int)) == _abi.CSSM_EINVAL_ARG
        assert b"cssm_fleet_ll_filter" in fl.lib.cssm_last_error()
        # still usable
        got = pmmh_native_fleet(um, inits, datas, n, 0.05, iters, seeds, fleet=fl)
        for k in range(3):
            assert_chain_equal(got, k, pmmh_native(um, inits[k], datas[k], n, 0.05, iters, seed=seeds[k]))
