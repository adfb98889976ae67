"""-m gpu: whole PMMH chains for LGCP fleets (cssm_fleet_pmmh_chains_lgcp, k_fleet_pmmh_lgcp): a chain per event stream, every iteration
and event of a chain in one launch, the transition coefficients over delta formed in the block once per iteration.

  * all priors flat and L = sqrt(0.3) I: bit for bit cssm_pmmh_run on an LGCP handle per chain (ll, theta, accepted, last_state);
  * a dense lower-triangular factor with a zero row, a NORMAL and a UNIFORM prior: bit for bit the sequential twin
    (pmmh_chain_twin.run_chain over pmmh_lgcp_twin.lgcp_ll_fn), with one factor and with one per chain;
  * the split over launches and a chain continued through first_iter / ll0 / state0 change no bit;
  * a chain whose stream cannot be weighed rejects everything and disturbs nobody;
  * more chains than compute units; the fleet is only lent (its predicted levels included); what needs a fleet to be refused.

Five streams at precision 2 on [0, 3] with 30, 7, 1, 12 and 0 events, seeds of their own.  Stream 0 repeats an event time (n_sub == 0);
stream 1 is the level fixture: under chain 1's start its filter keeps the predicted level at some events and rules it out at others
(``test_the_level_stream_takes_both_branches``).  There is no statistical acceptance test: no exact LGCP likelihood exists to hold a
posterior to; the decision logic is run_chain's (tests/test_pmmh_chains_host.py holds it to a quadrature) and the LGCP filter is held to
the oracle in tests/test_gpu_fleet_lgcp.py."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import cases
import pmmh_chain_twin as twin
import pmmh_lgcp_twin as lt
from composablestatespacemodels_amd import CssmError, _abi, load_library
from composablestatespacemodels_amd.filter import NativeLgcpFleet, NativePf, NativePfFleet
from composablestatespacemodels_amd.model import Model, Parameters, Sde, SdeParameter
from composablestatespacemodels_amd.pmmh import Prior, fleet_posterior_rows, pmmh_lgcp_fleet_chains
from oracle import oracle

pytestmark = pytest.mark.gpu

SEED = cases.SEED
P = lt.PRECISION
ITERS = 12
DELTA = 0.3
# the level stream: a first event at t0 (dt = 0), a repeated time, a long gap (the max falls), a short step behind it (the max rises back)
LEVEL = np.array([0.0, 0.05, 0.05, 0.3, 0.31, 2.81, 2.9])
STREAMS = (lt.stream30(), LEVEL, lt.stream(1, SEED + 5), lt.stream(12, SEED + 6), np.zeros(0))
S = len(STREAMS)


def d2_model():
    p = Parameters.apply(None, SdeParameter.ouParameter(0.1, 0.5, 0.4, [0.1, 0.15], 0.5))
    return Model.lgcp(Sde.ouProcess(2)).run(p)


MODELS = {"c4": cases.c4_model, "d2": d2_model, "seasonal": cases.lgcp_seasonal_model}


def seeds_of(count=S):
    return [SEED + 77 + 13 * k for k in range(count)]


def theta0_of(model, count=S):
    """a start per chain: the model's own, shifted a little; chain 1 (the level stream) with a high mean of the first component, so that
    a long gap's hazard moves the max by more than the prediction tolerates"""
    th = np.array(model.parameters().flattenParams())
    out = np.array([th + 0.01 * k for k in range(count)])
    if count > 1:
        out[1, 3] = 5.5                                           # slot 3: mu of the first (OU) component
    return out


def pack():
    off, t, _, _ = NativeLgcpFleet.pack(list(STREAMS), allow_empty=True)
    return off, t


def assert_chain_equal(got, want, k, what=""):
    for a, b, name in zip(got[:4], want[:4], ("ll", "theta", "accepted", "last_state")):
        np.testing.assert_array_equal(a[k], b, err_msg=f"{what} chain {k}: {name}")


def assert_no_events_chain(got, k):
    assert got[5][k] == _abi.CSSM_EINVAL_ARG and got[4][k].tolist() == [0, 0]
    assert np.isnan(got[0][k]).all() and np.isnan(got[1][k]).all() and np.isnan(got[3][k]).all() and (got[2][k] == -1).all()


# 0 ------------------------------------------------------------------------------------------------------------------------------
def test_the_level_stream_takes_both_branches():
    """a condition on the fixture, not a tolerance: under the FIRST PROPOSAL of chain 1 (what iteration 0 filters) the oracle keeps the
    predicted level at some events of the level stream and rules it out at others"""
    model = cases.c4_model()
    assert model.parameters().flattenParams()[3] == 0.1           # slot 3 is mu
    th0, seed, n = theta0_of(model)[1], seeds_of()[1], 100
    prop = twin.propose(math.sqrt(DELTA) * np.eye(5), twin.proposal_normals(seed, 0, 5), th0)
    desc = lt.unparam_of(model).run(model.parameters().withFlat(prop)).descriptor(P)
    o = oracle.OraclePf(desc, n, twin.filter_key(seed, 0))
    o.init(float(LEVEL[0]))
    kept = ruled_out = 0
    for s, t in enumerate(LEVEL):
        c = o.ref_level(1.0)
        o.step(float(t), 1.0, True)
        ref, gmax = o.ref()
        assert np.isnan(c) == (s == 0)
        kept += int(s > 0 and ref == c and c != gmax)
        ruled_out += int(s > 0 and ref == gmax and c != gmax)
    print(f"    level stream: prediction kept at {kept} events, ruled out at {ruled_out}")
    assert kept > 0 and ruled_out > 0 and LEVEL[2] == LEVEL[1]


# 1 ------------------------------------------------------------------------------------------------------------------------------
def handle_chain(model, n, seed, theta0, t, iters):
    """cssm_pmmh_run on an LGCP handle of n particles: (ll, theta, accepted, last_state)"""
    nt, d = len(theta0), model.dimension
    dp = C.POINTER(C.c_double)
    tt, y, h = lt.events(t)
    th0 = np.ascontiguousarray(theta0, dtype=np.float64)
    ll, th, acc, last = np.zeros(iters), np.zeros((iters, nt)), np.zeros(iters, dtype=np.int32), np.zeros((iters, d))
    with NativePf(model, n, seed, lgcp_precision=P) as pf:
        _abi.check(pf.lib.cssm_pmmh_run(pf._h, model.descriptor(P).ptr(), th0.ctypes.data_as(dp), nt, DELTA, tt.ctypes.data_as(dp), y.ctypes.data_as(dp),
                                        h.ctypes.data_as(C.POINTER(C.c_uint8)), len(tt), int(seed), iters, ll.ctypes.data_as(dp), th.ctypes.data_as(dp),
                                        acc.ctypes.data_as(C.POINTER(C.c_int32)), last.ctypes.data_as(dp)))
    return ll, th, acc, last


@pytest.mark.parametrize("n", [100, 1000, 1024, 4096])
@pytest.mark.parametrize("name", list(MODELS))
def test_flat_priors_and_an_isotropic_factor_are_cssm_pmmh_run_on_a_handle(name, n):
    model = MODELS[name]()
    theta0 = theta0_of(model)
    nt = theta0.shape[1]
    with NativeLgcpFleet(model, n, S, P) as fl:
        got = fl.pmmh_chains_lgcp(model.descriptor(P), theta0, math.sqrt(DELTA) * np.eye(nt), *pack(), seeds_of(), ITERS)
        assert fl.pmmh_chains_lgcp_last_ms() > 0.0
    assert list(got[5]) == [0, 0, 0, 0, _abi.CSSM_EINVAL_ARG] and not got[4].any()
    for k in range(4):
        assert_chain_equal(got, handle_chain(model, n, seeds_of()[k], theta0[k], STREAMS[k], ITERS), k, name)
        assert np.isfinite(got[0][k]).all()
    print(f"    {name} n = {n}: accepted of {ITERS}: {got[2][:4, -1].tolist()}")
    assert_no_events_chain(got, 4)


# 2 ------------------------------------------------------------------------------------------------------------------------------
DENSE_ITERS = 40


@functools.lru_cache(maxsize=None)
def twin_chains(name, n, per_chain, iters=DENSE_ITERS, first=0):
    model, L, priors = lt.dense_case(name)
    theta0 = theta0_of(model)
    out = []
    for k in range(4):
        ll_fn = lt.lgcp_ll_fn(lt.unparam_of(model), model.parameters(), n, STREAMS[k])
        Lk = L * (1.0 + 0.25 * k) if per_chain else L
        out.append(lt.run_chain(ll_fn, theta0[k], Lk, priors, seeds_of()[k], iters, model.dimension, first_iter=first))
    return out


@pytest.mark.parametrize("per_chain", [0, 1])
@pytest.mark.parametrize("name", ["c4", "seasonal"])
def test_a_dense_factor_and_priors_are_the_twin(name, per_chain):
    model, L, priors = lt.dense_case(name)
    n = 100
    theta0 = theta0_of(model)
    nt = theta0.shape[1]
    assert np.count_nonzero(np.tril(L, -1)) >= nt and not L[1].any() and L[3, 1] == 0.0 and L[3, 0] != 0.0 and L[3, 2] != 0.0
    chol = np.array([L * (1.0 + 0.25 * k) for k in range(S)]) if per_chain else L
    with NativeLgcpFleet(model, n, S, P) as fl:
        got = fl.pmmh_chains_lgcp(model.descriptor(P), theta0, chol, *pack(), seeds_of(), DENSE_ITERS, priors=priors)
    want = twin_chains(name, n, per_chain)
    accepted = by_decision = unfiltered = 0
    for k in range(4):
        assert_chain_equal(got, want[k], k, name)
        np.testing.assert_array_equal(got[4][k], want[k][4], err_msg=f"chain {k}: diag")
        np.testing.assert_array_equal(got[1][k][:, 1], np.full(DENSE_ITERS, theta0[k, 1]))    # the zero row: the slot's bits never change
        assert np.all((got[1][k][:, 4] >= priors[4].a) & (got[1][k][:, 4] <= priors[4].b))
        accepted += int(want[k][2][-1]); unfiltered += int(want[k][4][0])
        by_decision += DENSE_ITERS - int(want[k][2][-1]) - int(want[k][4][0])
    print(f"    {name}, per_chain = {per_chain}: the twin accepts {accepted}, rejects {by_decision} by the decision and {unfiltered} unfiltered")
    assert accepted > 0 and by_decision > 0 and unfiltered > 0    # all three outcomes occur, on the twin's own output
    assert_no_events_chain(got, 4)


# 3 ------------------------------------------------------------------------------------------------------------------------------
def test_the_split_over_launches_and_a_continued_chain_change_no_bit():
    model, L, priors = lt.dense_case("seasonal")
    n = 257
    theta0 = theta0_of(model)
    with NativeLgcpFleet(model, n, S, P) as fl:
        run = lambda **kw: fl.pmmh_chains_lgcp(model.descriptor(P), kw.pop("theta0", theta0), L, *pack(), seeds_of(), kw.pop("iters", ITERS),
                                               priors=priors, **kw)
        whole = run()
        for per in (1, 5):
            got = run(iters_per_launch=per)
            for a, b, what in zip(got, whole, ("ll", "theta", "accepted", "last_state", "diag", "rc")):
                np.testing.assert_array_equal(a, b, err_msg=f"{what}, {per} per launch")
        first = run(iters=7)
        live = slice(0, 4)
        th, l0, s0 = first[1][:, -1].copy(), first[0][:, -1].copy(), first[3][:, -1].copy()
        th[4], l0[4], s0[4] = theta0[4], -1e99, 0.0               # (the stream without events has NaN rows; it runs nothing)
        rest = run(theta0=th, iters=ITERS - 7, first_iter=7, ll0=l0, state0=s0)
    for i, what in ((0, "ll"), (1, "theta"), (3, "last_state")):
        np.testing.assert_array_equal(np.concatenate([first[i][live], rest[i][live]], axis=1), whole[i][live], err_msg=what)
    np.testing.assert_array_equal(np.concatenate([first[2][live], rest[2][live] + first[2][live, -1:]], axis=1), whole[2][live])
    np.testing.assert_array_equal(first[4] + rest[4], whole[4])
    assert 0 < whole[2][live, -1].max() <= ITERS


# 4 ------------------------------------------------------------------------------------------------------------------------------
def test_a_chain_whose_stream_cannot_be_weighed_rejects_everything_and_disturbs_nobody():
    model, n = cases.c4_model(), 100
    theta0 = theta0_of(model)
    wild = theta0.copy()
    wild[3] = np.array(Parameters.apply(None, SdeParameter.ouParameter(800, 0.5, 0.4, 800, 0.5)).flattenParams())
    L = 0.1 * np.eye(5)
    with NativeLgcpFleet(model, n, S, P) as fl:
        good = fl.pmmh_chains_lgcp(model.descriptor(P), theta0, L, *pack(), seeds_of(), ITERS)
        got = fl.pmmh_chains_lgcp(model.descriptor(P), wild, L, *pack(), seeds_of(), ITERS)
    assert got[4][3].tolist() == [0, ITERS] and not got[2][3].any() and np.all(got[0][3] == -1e99) and not got[3][3].any()
    np.testing.assert_array_equal(got[1][3], np.repeat(wild[3][None], ITERS, axis=0))
    assert list(got[5]) == list(good[5]) and not good[4].any()
    for k in (0, 1, 2):
        assert_chain_equal(got, [a[k] for a in good[:4]], k)
        assert got[4][k].tolist() == [0, 0]
    # ... and the neighbours are their twins
    for k in (0, 2):
        ll_fn = lt.lgcp_ll_fn(lt.unparam_of(model), model.parameters(), n, STREAMS[k])
        assert_chain_equal(got, lt.run_chain(ll_fn, theta0[k], L, None, seeds_of()[k], ITERS, 1), k, "twin")


# 5 ------------------------------------------------------------------------------------------------------------------------------
def test_more_chains_than_compute_units():
    model, n, chains, iters = cases.c4_model(), 64, 300, 6
    th = np.array(model.parameters().flattenParams())
    theta0 = np.array([th + 0.01 * (k % 150) for k in range(chains)])
    seeds = [SEED + 5 + 7 * (k % 150) for k in range(chains)]     # chains k and k + 150: equal seeds and starts
    t = STREAMS[3]
    L = math.sqrt(0.05) * np.eye(5)
    with NativeLgcpFleet(model, n, chains, P) as fl:
        off, tt, _, _ = fl.pack([t] * chains)
        got = fl.pmmh_chains_lgcp(model.descriptor(P), theta0, L, off, tt, seeds, iters)
    assert not got[5].any() and not got[4].any() and np.isfinite(got[0]).all()
    for a in got[:4]:
        np.testing.assert_array_equal(a[:150], a[150:])
    assert len({got[0][k].tobytes() for k in range(150)}) > 100   # ... and the others are chains of their own
    for k in (0, 149, 299):
        ll_fn = lt.lgcp_ll_fn(lt.unparam_of(model), model.parameters(), n, t)
        assert_chain_equal(got, lt.run_chain(ll_fn, theta0[k], L, None, seeds[k], iters, 1), k, "twin")


# 6 ------------------------------------------------------------------------------------------------------------------------------
def test_the_fleet_is_only_lent():
    model, L, priors = lt.dense_case("c4")
    n, live = 100, 4
    theta0 = theta0_of(model)[:live]
    times = [LEVEL[[0, 1, 3, 5, 6]] + 0.25 * k for k in range(live)]            # the gap of the level stream: a level worth predicting
    off, t, _, _ = NativeLgcpFleet.pack(list(STREAMS[:4]))
    with NativeLgcpFleet(model, n, live, P) as lent, NativeLgcpFleet(model, n, live, P) as kept:
        def stepped(fl, i):
            return fl.step(np.array([ts[i] for ts in times]), np.ones(live))
        for fl in (lent, kept):
            fl.reseed(seeds_of(live))
            fl.init(np.array([ts[0] for ts in times]))
            for i in (1, 2):
                assert not stepped(fl, i)[2].any()
        before = [(lent.particles(k), lent.ancestors(k), lent.observation_index(k)) for k in range(live)]
        out = lent.pmmh_chains_lgcp(model.descriptor(P), theta0, L, off, t, [7] * live, ITERS, priors=priors)
        assert not out[5].any() and np.isfinite(out[0]).all()
        for k in range(live):
            np.testing.assert_array_equal(lent.particles(k), before[k][0]); np.testing.assert_array_equal(lent.ancestors(k), before[k][1])
            assert lent.observation_index(k) == before[k][2] == 2
        for i in (3, 4):                                          # ll, ESS, clocks, keys, parameters and the predicted level: the undisturbed fleet's
            a, b = stepped(lent, i), stepped(kept, i)
            for u, v in zip(a, b):
                np.testing.assert_array_equal(u, v)
        for k in range(live):
            np.testing.assert_array_equal(lent.particles(k), kept.particles(k)); np.testing.assert_array_equal(lent.ancestors(k), kept.ancestors(k))
            assert lent.observation_index(k) == kept.observation_index(k) == 4


# 7 ------------------------------------------------------------------------------------------------------------------------------
def test_what_needs_a_fleet_to_be_refused():
    c4, c2 = cases.c4_model(), cases.c2_model()
    th = np.repeat(np.array(c4.parameters().flattenParams())[None], 2, axis=0)
    off, t, _, _ = NativeLgcpFleet.pack([np.arange(3.0)] * 2)
    with NativePfFleet(c2, 64, 2) as fl:                          # a plain fleet: sent to the call that runs its chains
        lgcp_call = functools.partial(NativeLgcpFleet.pmmh_chains_lgcp, fl)
        fl.n_theta = 5                                            # (the Python side checks the row length against the fleet's own model)
        with pytest.raises(CssmError, match="cssm_fleet_pmmh_chains_lgcp: the fleet was not made by cssm_fleet_create_lgcp") as e:
            lgcp_call(c4.descriptor(P), th, 0.1 * np.eye(5), off, t, [1, 2], 1)
        assert e.value.code == _abi.CSSM_EINVAL_ARG and "cssm_fleet_pmmh_chains runs" in str(e.value)
    with NativeLgcpFleet(c4, 64, 2, P) as fl:
        with pytest.raises(CssmError, match="not of the fleet's model structure") as e:         # another precision: another structure
            fl.pmmh_chains_lgcp(c4.descriptor(3), th, 0.1 * np.eye(5), off, t, [1, 2], 1)
        assert e.value.code == _abi.CSSM_EINVAL_DESC
        with pytest.raises(CssmError, match="not of the fleet's model structure") as e:
            fl.n_theta = 11
            fl.pmmh_chains_lgcp(cases.lgcp_seasonal_model().descriptor(P), np.zeros((2, 11)), 0.1 * np.eye(11), off, t, [1, 2], 1)
        assert e.value.code == _abi.CSSM_EINVAL_DESC
        fl.n_theta = 5
        pri = [Prior.flat()] * 5
        pri[1] = Prior.uniform(th[0, 1] + 1.0, th[0, 1] + 2.0)
        with pytest.raises(CssmError, match="outside the prior's support") as e:
            fl.pmmh_chains_lgcp(c4.descriptor(P), th, 0.1 * np.eye(5), off, t, [1, 2], 1, priors=pri)
        assert e.value.code == _abi.CSSM_EINVAL_ARG and "chain 0" in str(e.value)
        chol = np.array([0.1 * np.eye(5)] * 2); chol[1, 2, 4] = 0.5
        with pytest.raises(CssmError, match=r"chol 1 \[2\]\[4\]"):
            fl.pmmh_chains_lgcp(c4.descriptor(P), th, chol, off, t, [1, 2], 1)
        lib = load_library()
        bad = np.array([0, 3, 2], dtype=np.uint64)
        p = lambda a, ty: a.ctypes.data_as(C.POINTER(ty))
        z, L, seeds, rc, acc = np.zeros(40), 0.1 * np.eye(5), np.zeros(2, dtype=np.uint64), np.zeros(2, dtype=np.int32), np.zeros(2, dtype=np.int32)
        got = lib.cssm_fleet_pmmh_chains_lgcp(fl._h, c4.descriptor(P).ptr(), p(th, C.c_double), 5, p(L, C.c_double), 0, None, None, None, 0, 1, 0,
                                              p(seeds, C.c_uint64), p(bad, C.c_uint64), p(z, C.c_double), p(z, C.c_double), p(z, C.c_double),
                                              p(acc, C.c_int32), p(z, C.c_double), None, p(rc, C.c_int))
        assert got == _abi.CSSM_EINVAL_ARG and b"off must be non-decreasing" in lib.cssm_last_error()
        with pytest.raises(CssmError, match="no chains have run"):
            fl.pmmh_chains_lgcp_last_ms()
        # the plain call keeps refusing the LGCP fleet, and the fleet is still usable
        fl.n_theta = 4
        with pytest.raises(CssmError, match="cssm_fleet_pmmh_chains: an LGCP fleet filters event streams"):
            fl.pmmh_chains(cases.linear_model().descriptor(), np.zeros((2, 4)), 0.1 * np.eye(4), off, t, np.ones(len(t)),
                           np.ones(len(t), dtype=np.uint8), [1, 2], 1)
        fl.n_theta = 5
        with pytest.raises(CssmError, match="LGCP observation model") as e:                   # (its LGCP descriptor: before the fleet is looked at)
            fl.pmmh_chains(c4.descriptor(P), th, 0.1 * np.eye(5), off, t, np.ones(len(t)), np.ones(len(t), dtype=np.uint8), [1, 2], 1)
        assert e.value.code == _abi.CSSM_EINVAL_DESC
        out = fl.pmmh_chains_lgcp(c4.descriptor(P), th, 0.2 * np.eye(5), off, t, [1, 2], 2)
        assert not out[5].any() and np.isfinite(out[0]).all() and fl.pmmh_chains_lgcp_last_ms() > 0.0


def test_the_python_entry_point_returns_what_the_posterior_helpers_take():
    um, p0 = lt.unparam_of(cases.c4_model()), cases.c4_model().parameters()
    inits = [p0.withFlat(np.array(p0.flattenParams()) + 0.01 * k) for k in range(3)]
    t, seeds, n = STREAMS[3], [3, 4, 5], 100
    L = math.sqrt(DELTA) * np.eye(5)
    got = pmmh_lgcp_fleet_chains(um, inits, t, n, P, L, iters=ITERS, seeds=seeds)
    assert len(got) == 5 and got[4].shape == (3, 2) and not got[4].any()
    for k in range(3):
        assert_chain_equal(got, handle_chain(cases.c4_model(), n, seeds[k], np.array(inits[k].flattenParams()), t, ITERS), k)
    rows = fleet_posterior_rows(got[1], got[3], burn_in=2, thin=2)
    assert len(rows) == 3 and rows[0][0].shape == (5, 5) and rows[0][1].shape == (5, 1)
    # one stream per chain, named priors, another launch length, a fleet of the caller's: no bit changes
    with NativeLgcpFleet(cases.c4_model(), n, 3, P) as fl:
        per = pmmh_lgcp_fleet_chains(um, inits, [t, t, t], n, P, L, priors={"0.phi[0]": Prior.flat()}, iters=ITERS, seeds=seeds, iters_per_launch=5,
                                     fleet=fl)
        with pytest.raises(ValueError, match="the run needs"):
            pmmh_lgcp_fleet_chains(um, inits, t, n, 3, L, iters=1, seeds=seeds, fleet=fl)
    for a, b in zip(per, got):
        np.testing.assert_array_equal(a, b)
    with pytest.raises(ValueError, match="one seed per chain"):
        pmmh_lgcp_fleet_chains(um, inits, t, n, P, L, iters=1, seeds=[1])
    with pytest.raises(ValueError, match="no records"):
        pmmh_lgcp_fleet_chains(um, inits, [t, np.zeros(0), t], n, P, L, iters=1, seeds=seeds)
