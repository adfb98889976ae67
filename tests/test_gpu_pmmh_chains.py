"""-m gpu: whole PMMH chains on the device (cssm_fleet_pmmh_chains, k_fleet_pmmh): a chain per series, every iteration and record of a
chain in one launch, the record built in the block from the chain's own parameter row.

  * all priors flat and a diagonal factor: bit for bit cssm_fleet_pmmh_run on the same fleet (ll, theta, accepted, last_state) -- the
    records the block builds are the host's;
  * a full lower-triangular factor with a zero row, NORMAL and UNIFORM priors: bit for bit the sequential twin (pmmh_chain_twin.py),
    with one factor and with one per chain; proposals outside a tight UNIFORM bound are counted and repeat the row before;
  * the split over launches and a chain continued through first_iter / ll0 / state0 change no bit;
  * a chain whose filter never has a usable weight rejects everything and disturbs nobody;
  * the fleet is only lent; what needs a fleet to be refused.

Five chains with seeds of their own on ragged data (1, 7 and 30 records, records with has_obs = 0; every series' first record is at
dt = 0, the series' smallest time), six iterations unless said."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import cases
import pmmh_chain_twin as twin
from composablestatespacemodels_amd import CssmError, _abi, load_library
from composablestatespacemodels_amd.filter import NativeLgcpFleet, NativePfFleet
from composablestatespacemodels_amd.pmmh import Prior
import test_pmmh_chains_host as H
import test_smc2_host as sm
from composablestatespacemodels_amd import pmmh
from test_pmmh_chains_host import unparam_of

pytestmark = pytest.mark.gpu

SEED = cases.SEED
ITERS = 6
LENGTHS = (7, 30, 1, 12, 0)                                      # series 4 has no records
MODELS = {"c1": cases.c1_model, "c2": cases.c2_model, "linear": cases.linear_model, "studentt": cases.studentt_model, "c3": cases.c3_model}
GAUSSIAN = ("linear", "studentt")


def seeds_of(S):
    return [SEED + 77 + 13 * k for k in range(S)]


@functools.lru_cache(maxsize=None)
def series_of(name):
    """five ragged series of the model's kind; series 0 and 1 have unobserved records"""
    t, y, has = cases.gaussian_series(40, seed=SEED + 5) if name in GAUSSIAN else cases.poisson_counts(40, seed=SEED + 5)
    datas = []
    for k, T in enumerate(LENGTHS):
        a = 3 * k
        hk = np.ones(T, dtype=np.uint8)
        if k == 0:
            hk[[2, 3]] = 0
        if k == 1:
            hk[[0, 11, 29]] = 0
        datas.append((t[a:a + T].copy(), y[a:a + T].copy(), hk))
    return datas


def theta0_of(model, S):
    th = np.array(model.parameters().flattenParams())
    return np.array([th + 0.01 * k for k in range(S)])


def pack(datas):
    return NativePfFleet.pack(datas, allow_empty=True)


def assert_rows_equal(got, want, k, what=""):
    for a, b, name in zip(got[:4], want[:4], ("ll", "theta", "accepted", "last_state")):
        np.testing.assert_array_equal(a[k], b[k] if np.ndim(b) == np.ndim(a) else b, err_msg=f"{what} chain {k}: {name}")


# 5 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [100, 1000, 1024, 4096])
@pytest.mark.parametrize("name", list(MODELS))
def test_flat_priors_and_a_diagonal_factor_are_cssm_fleet_pmmh_run(name, n):
    model, datas = MODELS[name](), series_of(name)
    S, delta = len(datas), 0.02
    theta0 = theta0_of(model, S)
    nt = theta0.shape[1]
    filled = list(datas[:4]) + [datas[0]]                         # (cssm_fleet_pmmh_run refuses a series without records)
    with NativePfFleet(model, n, S) as fl:
        want = fl.pmmh_run(model.descriptor(), theta0, delta, *NativePfFleet.pack(filled), seeds_of(S), ITERS)
        got = fl.pmmh_chains(model.descriptor(), theta0, math.sqrt(delta) * np.eye(nt), *pack(datas), seeds_of(S), ITERS)
        assert fl.pmmh_chains_last_ms() > 0.0
    assert list(got[5]) == [0, 0, 0, 0, _abi.CSSM_EINVAL_ARG] and not got[4].any()
    for k in range(4):
        assert_rows_equal(got, want, k, name)
        assert np.isfinite(got[0][k]).all()
    print(f"    {name} n = {n}: accepted of {ITERS}: {want[2][:4, -1].tolist()}")
    assert np.isnan(got[0][4]).all() and np.isnan(got[1][4]).all() and np.isnan(got[3][4]).all() and (got[2][4] == -1).all()


# 6 ------------------------------------------------------------------------------------------------------------------------------
def correlated_case():
    """C2 (n_theta = 10): a full lower-triangular factor with a zero row, a NORMAL and a UNIFORM prior (the bound tight enough that
    proposals fall outside)."""
    model = cases.c2_model()
    nt = 10
    rng = np.random.default_rng(SEED + 9)
    L = np.tril(rng.uniform(-0.03, 0.03, size=(nt, nt))) + 0.05 * np.eye(nt)
    L[3, :] = 0.0                                                 # slot 3 stays fixed
    L[7, 2] = 0.0                                                 # a zero inside a row is skipped
    th = np.array(model.parameters().flattenParams())
    priors = [Prior.flat()] * nt
    priors[2] = Prior.normal(th[2] + 0.1, 0.2)
    priors[4] = Prior.uniform(th[4] - 0.03, th[4] + 0.08)
    priors[9] = Prior.normal(th[9], 0.5)
    return model, L, priors


@functools.lru_cache(maxsize=None)
def twin_chains(n, per_chain):
    model, L, priors = correlated_case()
    datas = series_of("c2")
    S = len(datas)
    theta0 = theta0_of(model, S)
    out = []
    for k in range(4):
        ll_fn = twin.oracle_ll_fn(unparam_of(model), model.parameters(), n, *datas[k])
        Lk = L * (1.0 + 0.25 * k) if per_chain else L
        out.append(twin.run_chain(ll_fn, theta0[k], Lk, priors, seeds_of(S)[k], ITERS, model.dimension))
    return out


@pytest.mark.parametrize("per_chain", [0, 1])
def test_a_correlated_factor_and_priors_are_the_twin(per_chain):
    model, L, priors = correlated_case()
    datas = series_of("c2")
    S, n = len(datas), 100
    theta0 = theta0_of(model, S)
    chol = np.array([L * (1.0 + 0.25 * k) for k in range(S)]) if per_chain else L
    with NativePfFleet(model, n, S) as fl:
        got = fl.pmmh_chains(model.descriptor(), theta0, chol, *pack(datas), seeds_of(S), ITERS, priors=priors)
    want = twin_chains(n, per_chain)
    outside = 0
    for k in range(4):
        for a, b, what in zip(got[:4], want[k][:4], ("ll", "theta", "accepted", "last_state")):
            np.testing.assert_array_equal(a[k], b, err_msg=f"chain {k}: {what}")
        np.testing.assert_array_equal(got[4][k], want[k][4], err_msg=f"chain {k}: diag")
        np.testing.assert_array_equal(got[1][k][:, 3], np.full(ITERS, theta0[k, 3]))          # the zero row: the slot's bits never change
        lo, hi = priors[4].a, priors[4].b
        assert np.all((got[1][k][:, 4] >= lo) & (got[1][k][:, 4] <= hi))
        outside += int(got[4][k][0])
        # an iteration whose proposal fell outside repeats the row before: found again from the twin's own proposals
        cur = theta0[k]
        for q in range(ITERS):
            Lk = chol[k] if per_chain else chol
            prop = twin.propose(Lk, twin.proposal_normals(seeds_of(S)[k], q, 10), cur)
            if not (lo <= prop[4] <= hi):
                np.testing.assert_array_equal(got[1][k][q], cur)
                if q:
                    assert got[0][k][q] == got[0][k][q - 1] and got[2][k][q] == got[2][k][q - 1]
                    np.testing.assert_array_equal(got[3][k][q], got[3][k][q - 1])
            cur = got[1][k][q]
    assert outside > 0                                            # the bound is tight enough
    assert all(got[4][k][0] > 0 for k in range(4) if want[k][4][0] > 0) and got[4][4].tolist() == [0, 0]


# 7 ------------------------------------------------------------------------------------------------------------------------------
def test_the_split_over_launches_and_a_continued_chain_change_no_bit():
    model, L, priors = correlated_case()
    datas = series_of("c2")
    S, n = len(datas), 257
    theta0 = theta0_of(model, S)
    with NativePfFleet(model, n, S) as fl:
        run = lambda **kw: fl.pmmh_chains(model.descriptor(), kw.pop("theta0", theta0), L, *pack(datas), seeds_of(S), kw.pop("iters", ITERS),
                                          priors=priors, **kw)
        whole = run()
        for per in (1, 4):
            got = run(iters_per_launch=per)
            for a, b, what in zip(got, whole, ("ll", "theta", "accepted", "last_state", "diag", "rc")):
                np.testing.assert_array_equal(a, b, err_msg=f"{what}, {per} per launch")
        first = run(iters=4)
        live = slice(0, 4)
        th, l0, s0 = first[1][:, -1].copy(), first[0][:, -1].copy(), first[3][:, -1].copy()
        th[4], l0[4], s0[4] = theta0[4], -1e99, 0.0               # (the series without records has NaN rows; it runs nothing)
        rest = run(theta0=th, iters=2, first_iter=4, ll0=l0, state0=s0)
    for i, what in ((0, "ll"), (1, "theta"), (3, "last_state")):
        np.testing.assert_array_equal(np.concatenate([first[i][live], rest[i][live]], axis=1), whole[i][live], err_msg=what)
    np.testing.assert_array_equal(np.concatenate([first[2][live], rest[2][live] + first[2][live, -1:]], axis=1), whole[2][live])
    np.testing.assert_array_equal(first[4] + rest[4], whole[4])
    assert 0 < whole[2][live, -1].min() and whole[2][live, -1].max() <= ITERS


# 8 ------------------------------------------------------------------------------------------------------------------------------
def test_a_chain_without_a_usable_weight_rejects_everything_and_disturbs_nobody():
    model, datas = cases.linear_model(), series_of("linear")
    S, n = len(datas), 100
    theta0 = theta0_of(model, S)
    bad = [tuple(a.copy() for a in d) for d in datas]
    bad[1][1][5] = 1e200                                          # every particle's squared residual overflows: no usable weight
    L = 0.1 * np.eye(4)
    with NativePfFleet(model, n, S) as fl:
        good = fl.pmmh_chains(model.descriptor(), theta0, L, *pack(datas), seeds_of(S), ITERS)
        got = fl.pmmh_chains(model.descriptor(), theta0, L, *pack(bad), seeds_of(S), ITERS)
    assert got[4][1].tolist() == [0, ITERS] and not got[2][1].any() and np.all(got[0][1] == -1e99) and not got[3][1].any()
    np.testing.assert_array_equal(got[1][1], np.repeat(theta0[1][None], ITERS, axis=0))
    assert list(got[5]) == list(good[5]) and not good[4].any()
    for k in (0, 2, 3):
        assert_rows_equal(got, good, k)
        assert got[4][k].tolist() == [0, 0]


# 9 ------------------------------------------------------------------------------------------------------------------------------
def test_the_fleet_is_only_lent():
    model, L, priors = correlated_case()
    datas = series_of("c2")[:4]
    S, n = 4, 100
    theta0 = theta0_of(model, S)
    t, y, _ = cases.poisson_counts(4, seed=SEED + 1)
    with NativePfFleet(model, n, S) as lent, NativePfFleet(model, n, S) as kept:
        def stepped(fl, i):
            return fl.step(np.full(S, t[i]), y[i] + np.arange(S, dtype=np.float64))
        for fl in (lent, kept):
            fl.reseed(seeds_of(S))
            fl.init(np.full(S, t[0]))
            for i in (0, 1):
                assert not stepped(fl, i)[2].any()
        before = [(lent.particles(k), lent.ancestors(k), lent.observation_index(k)) for k in range(S)]
        out = lent.pmmh_chains(model.descriptor(), theta0, L, *pack(datas), [7] * S, ITERS, priors=priors)
        assert not out[5].any() and np.isfinite(out[0]).all()
        for k in range(S):
            np.testing.assert_array_equal(lent.particles(k), before[k][0]); np.testing.assert_array_equal(lent.ancestors(k), before[k][1])
            assert lent.observation_index(k) == before[k][2] == 2
        for i in (2, 3):                                          # ll, ESS, clocks, keys and parameters: the stepped fleet is the undisturbed one
            a, b = stepped(lent, i), stepped(kept, i)
            for u, v in zip(a, b):
                np.testing.assert_array_equal(u, v)
        for k in range(S):
            np.testing.assert_array_equal(lent.particles(k), kept.particles(k)); np.testing.assert_array_equal(lent.ancestors(k), kept.ancestors(k))
            assert lent.observation_index(k) == kept.observation_index(k) == 4


def test_what_needs_a_fleet_to_be_refused():
    lin, c2 = cases.linear_model(), cases.c2_model()
    datas = [(np.arange(3.0), np.ones(3), None)] * 2
    off, t, y, has = NativePfFleet.pack(datas)
    with NativeLgcpFleet(cases.c4_model(), 64, 2, 2) as fl:     # an LGCP fleet, by name, naming who serves it
        fl.n_theta = 4                                          # (the Python side checks the row length against the fleet's own model)
        with pytest.raises(CssmError, match="cssm_fleet_pmmh_chains: an LGCP fleet filters event streams") as e:
            fl.pmmh_chains(lin.descriptor(), np.zeros((2, 4)), 0.1 * np.eye(4), off, t, y, has, [1, 2], 1)
        assert e.value.code == _abi.CSSM_EINVAL_ARG and "cssm_pmmh_run_batched" in str(e.value)
    with NativePfFleet(c2, 64, 2) as fl:
        with pytest.raises(CssmError, match="LGCP") as e:       # an LGCP descriptor: before the fleet is looked at
            fl.n_theta = 5
            fl.pmmh_chains(cases.c4_model().descriptor(), np.zeros((2, 5)), 0.1 * np.eye(5), off, t, y, has, [1, 2], 1)
        assert e.value.code == _abi.CSSM_EINVAL_DESC and "cssm_pmmh_run_batched" in str(e.value)
        fl.n_theta = 4
        with pytest.raises(CssmError, match="not of the fleet's model structure") as e:
            fl.pmmh_chains(lin.descriptor(), np.zeros((2, 4)), 0.1 * np.eye(4), off, t, y, has, [1, 2], 1)
        assert e.value.code == _abi.CSSM_EINVAL_DESC
        fl.n_theta = 10
        th = np.repeat(np.array(c2.parameters().flattenParams())[None], 2, axis=0)
        pri = [Prior.flat()] * 10
        pri[1] = Prior.uniform(th[0, 1] + 1.0, th[0, 1] + 2.0)
        with pytest.raises(CssmError, match="outside the prior's support") as e:
            fl.pmmh_chains(c2.descriptor(), th, 0.1 * np.eye(10), off, t, y, has, [1, 2], 1, priors=pri)
        assert e.value.code == _abi.CSSM_EINVAL_ARG
        chol = np.array([0.1 * np.eye(10)] * 2); chol[1, 2, 5] = 0.5
        with pytest.raises(CssmError, match=r"chol 1 \[2\]\[5\]"):
            fl.pmmh_chains(c2.descriptor(), th, chol, off, t, y, has, [1, 2], 1)
        lib = load_library()
        bad = np.array([0, 3, 2], dtype=np.uint64)
        p = lambda a, ty: a.ctypes.data_as(C.POINTER(ty))
        z, L, seeds, rc, acc = np.zeros(40), 0.1 * np.eye(10), np.zeros(2, dtype=np.uint64), np.zeros(2, dtype=np.int32), np.zeros(2, dtype=np.int32)
        got = lib.cssm_fleet_pmmh_chains(fl._h, c2.descriptor().ptr(), p(th, C.c_double), 10, p(L, C.c_double), 0, None, None, None, 0, 1, 0,
                                         p(seeds, C.c_uint64), p(bad, C.c_uint64), p(z, C.c_double), p(z, C.c_double), None, p(z, C.c_double),
                                         p(z, C.c_double), p(acc, C.c_int32), p(z, C.c_double), None, p(rc, C.c_int))
        assert got == _abi.CSSM_EINVAL_ARG and b"off must be non-decreasing" in lib.cssm_last_error()
        with pytest.raises(CssmError, match="no chains have run"):
            fl.pmmh_chains_last_ms()
        out = fl.pmmh_chains(c2.descriptor(), th, 0.05 * np.eye(10), off, t, y, has, [1, 2], 2)     # still usable
        assert not out[5].any() and np.isfinite(out[0]).all() and fl.pmmh_chains_last_ms() > 0.0


# 10 -----------------------------------------------------------------------------------------------------------------------------
def test_the_chains_on_the_device_recover_the_exact_posterior():
    """tests/test_pmmh_chains_host.py's truth configuration -- its model, data, priors, seeds, pilot, CHAINS x ITERS and burn-in -- with the
    particle filter (N = 200) in place of the exact likelihood: PMMH is exact for any N, so the quadrature is the truth, not an
    approximation.  The pilot and the tuned chains are two calls on one fleet, the second continued through first_iter / ll0 / state0 with
    a factor per chain (chol_from_pilot of the chain's own pilot).  The test prints every z before it asserts.  Measured on one MI355X
    (no seed retried or dropped): acceptance rates 0.25 - 0.38, z of (mean log obs sd, mean log sigma, sd, sd) against the quadrature
    -1.54, 0.41, 1.25, 0.51 (accepted); against the prior's moments -68.8, 23.3, -29.1, -24.3 (rejected).  The tuned chains' call takes
    267 ms on the device, the test 3 s."""
    S, n = H.CHAINS, 200
    um, base = sm.unparam(), sm.base_params()
    t, y, has = cases.gaussian_series(sm.T)
    packed = NativePfFleet.pack([(t, y, has)] * S)
    seeds = [H.truth_seed(k) for k in range(S)]
    desc = um.run(base).descriptor()
    with NativePfFleet(um.run(base), n, S) as fl:
        pilot = fl.pmmh_chains(desc, np.repeat(H.truth_start()[None], S, axis=0), H.pilot_factor(), *packed, seeds, H.PILOT, priors=H.truth_priors())
        chol = np.array([pmmh.chol_from_pilot(pilot[1][k][H.PILOT // 4:]) for k in range(S)])
        out = fl.pmmh_chains(desc, pilot[1][:, -1], chol, *packed, seeds, H.ITERS, priors=H.truth_priors(), first_iter=H.PILOT,
                             ll0=pilot[0][:, -1], state0=pilot[3][:, -1])
        print(f"    device ms of the tuned chains' call: {fl.pmmh_chains_last_ms():.1f}")
    assert not out[5].any() and not out[4].any()
    rates = out[2][:, -1] / H.ITERS
    print(f"    acceptance rates {np.round(rates, 2).tolist()}")
    ref, err = sm.exact_cached()
    stats = H.chain_statistics(out[1])
    ok = H.judged(stats, ref[:4], err[:4], "pmmh on the device, N = 200")
    prior_ok = H.judged(stats, H.PRIOR_MOMENTS, err[:4], "against the prior's moments")
    assert ok and not prior_ok
    assert rates.min() > 0.05 and rates.max() < 0.7


def test_the_python_entry_point_returns_what_the_posterior_helpers_take():
    from composablestatespacemodels_amd import Data
    from composablestatespacemodels_amd.pmmh import fleet_posterior_rows, pmmh_fleet_chains, pmmh_native_fleet
    um, p0 = cases.c2_unparam(), cases.c2_params()
    inits = [p0.withFlat(np.array(p0.flattenParams()) + 0.01 * k) for k in range(3)]
    t, y, has = cases.poisson_counts(9, seed=SEED + 2, missing=0.2)
    data = [Data(float(a), float(b) if h else None) for a, b, h in zip(t, y, has)]
    seeds, delta = [3, 4, 5], 0.02
    want = pmmh_native_fleet(um, inits, data, 100, delta, ITERS, seeds)
    got = pmmh_fleet_chains(um, inits, data, 100, math.sqrt(delta) * np.eye(10), iters=ITERS, seeds=seeds)
    assert len(got) == 5 and got[4].shape == (3, 2) and not got[4].any()
    for a, b in zip(got[:4], want):
        np.testing.assert_array_equal(a, b)
    rows = fleet_posterior_rows(got[1], got[3], burn_in=2, thin=2)
    assert len(rows) == 3 and rows[0][0].shape == (2, 10) and rows[0][1].shape == (2, 3)
    named = pmmh_fleet_chains(um, inits, data, 100, math.sqrt(delta) * np.eye(10), priors={"0.phi[0]": Prior.normal(0.0, 10.0)}, iters=ITERS,
                              seeds=seeds, iters_per_launch=2)
    assert named[0].shape == (3, ITERS) and np.isfinite(named[0]).all()
    with pytest.raises(ValueError, match="one seed per chain"):
        pmmh_fleet_chains(um, inits, data, 100, np.eye(10), iters=1, seeds=[1])
