"""cssm_fleet_if2 (include/cssm_pf.h; an EXTENSION): iterated filtering, a search per series of a fleet, every iteration in one launch.
Against the sequential twin of the contract's section (tests/cpp/if2_twin.c; tests/test_fleet_if2_host.py ties it to the oracle):

  * theta_mean, ll, the final swarm, the last iteration's ll_t / ess_t / cloud / ancestors and the statuses bit for bit, at the scan,
    carry and padding edges of N, at d = 1, 3 and 16 and for every non-LGCP observation kind, on five ragged series (one without
    records, one with unobserved records, one with a repeated time);
  * a frozen swarm (every rw_sd = 0, one iteration) is the plain cssm_fleet_ll_filter of the same fleet under the iteration's key;
  * the result does not depend on how the iterations are split over launches, and a search continued from its swarm is the
    uninterrupted one; the fleet is only lent; one failing series does not disturb the others; an LGCP fleet is refused by name;
  * the acceptance configuration of the host file, once on the device: equal to the twin, hence inside the likelihood-ratio region."""
import ctypes as C

import numpy as np
import pytest

import cases
import test_fleet_if2_host as H
from composablestatespacemodels_amd import CssmError, _abi, load_library
from composablestatespacemodels_amd.filter import NativeLgcpFleet, NativePfFleet

pytestmark = pytest.mark.gpu
SEED = cases.SEED
LENGTHS = (9, 0, 12, 7, 10)
MODELS = {"c1": cases.c1_model, "c2": cases.c2_model, "maxdim": cases.max_dim_model}


def model_and_series(name):
    """(model, five ragged series): windows of one long series of the model's kind; series 1 has no records, series 2 unobserved records,
    series 3 a repeated time (dt = 0)."""
    if name in MODELS:
        model, (t, y, has) = MODELS[name](), cases.poisson_counts(16)
    else:
        model, t, y, has = cases.literal_case(name, 16)
    datas = []
    for k, T in enumerate(LENGTHS):
        a = (2 * k) % 4
        tk, yk, hk = t[a:a + T].copy(), y[a:a + T].copy(), np.ones(T, dtype=np.uint8)
        if k == 2:
            hk[[1, 2, 7]] = 0
        if k == 3:
            tk[4] = tk[3]
        datas.append((tk, yk, hk))
    return model, datas


def seeds_of(S):
    return [SEED + 101 * k for k in range(S)]


def assert_equal_to_twin(model, n, datas, out, sd, cool, iters, seeds, theta0):
    for k, data in enumerate(datas):
        want = H.twin_search(model, n, data, sd, cool, iters, seeds[k], theta0=theta0[k])
        assert out["rc"][k] == want["rc"], (k, out["rc"][k], want["rc"])
        np.testing.assert_array_equal(out["theta_mean"][k], want["theta_mean"], err_msg=f"series {k}")
        np.testing.assert_array_equal(out["ll"][k], want["ll"], err_msg=f"series {k}")
        np.testing.assert_array_equal(out["swarm"][k], want["swarm"], err_msg=f"series {k}")
        np.testing.assert_array_equal(out["ll_t"][k], want["ll_t"]); np.testing.assert_array_equal(out["ess_t"][k], want["ess_t"])
        np.testing.assert_array_equal(out["x"][k], want["x"]); np.testing.assert_array_equal(out["anc"][k], want["anc"])
        if len(data[0]):
            assert np.isfinite(out["theta_mean"][k]).all() and np.isfinite(out["ll"][k]).all()


EDGES = [1, 2, 63, 64, 65, 100, 257, 1000, 4095, 4096]      # DESIGN.md, "Which instantiations the suite runs": scan, carry and padding edges
# (2049, added below: the smallest N at which a whole wave of the block owns no particle)
KINDS = ["linear", "negbin", "zip", "bernoulli", "studentt", "beta", "gbsg", "euler", "c3"]
CASES = [("c2", n) for n in EDGES + [2049]] + [("c1", 65), ("c1", 100), ("maxdim", 100), ("maxdim", 257)] + [(name, 100) for name in KINDS]


@pytest.mark.parametrize("name,n", CASES)
def test_the_device_is_the_twin(name, n):
    model, datas = model_and_series(name)
    S, iters = len(datas), 2 if n >= 1000 else 3
    th = H.theta_of(model)
    theta0 = np.array([th + 0.01 * k for k in range(S)])
    sd = np.full(len(th), 0.02)
    sd[len(th) // 2] = 0.0                                       # one slot stays fixed
    with NativePfFleet(model, n, S) as fl:
        out = fl.if2(model.descriptor(), datas, sd, 0.5, iters, seeds_of(S), theta0=theta0, want_swarm=True, want_last=True)
        assert fl.if2_last_ms() > 0.0
    assert list(out["rc"]) == [0] * S
    assert np.isnan(out["theta_mean"][1]).all() and np.isnan(out["ll"][1]).all()          # no records: untouched, NaN rows
    np.testing.assert_array_equal(out["swarm"][1], np.repeat(theta0[1][:, None], n, axis=1))
    assert_equal_to_twin(model, n, datas, out, sd, 0.5, iters, seeds_of(S), theta0)


@pytest.mark.parametrize("d", list(range(1, 17)))
def test_every_latent_dimension(d):
    """k_fleet_if2<D> for every D: S = 3, N = 257, six records, two of them unweighted (the shape the other fleet kernels' tests run)."""
    model = cases.dim_model(d)
    t, y, has = cases.poisson_counts(6)
    has = has.copy(); has[[2, 4]] = 0
    datas = [(t, y, has), (t[:4], y[:4], has[:4]), (t[1:], y[1:], np.ones(5, dtype=np.uint8))]
    th = H.theta_of(model)
    theta0 = np.array([th - 0.02 * k for k in range(3)])
    sd = np.full(len(th), 0.03)
    with NativePfFleet(model, 257, 3) as fl:
        out = fl.if2(model.descriptor(), datas, sd, 0.5, 2, seeds_of(3), theta0=theta0, want_swarm=True, want_last=True)
    assert not out["rc"].any()
    assert_equal_to_twin(model, 257, datas, out, sd, 0.5, 2, seeds_of(3), theta0)


@pytest.mark.parametrize("name", ["c1", "c2", "linear"])
def test_a_frozen_swarm_is_the_plain_fleet_filter(name):
    model, datas = model_and_series(name)
    datas = [d for d in datas if len(d[0])]                     # (the plain filter gives a series without records a status of its own)
    S, n = len(datas), 300
    lib = load_library()
    th = H.theta_of(model)
    with NativePfFleet(model, n, S) as fl:
        fl.reseed([int(lib.cssm_pf_run_key(s, 1)) for s in seeds_of(S)])
        ll, ll_t, ess_t, rc = fl.ll_filter(datas)
        assert not rc.any()
        parts, ancs = [fl.particles(k) for k in range(S)], [fl.ancestors(k) for k in range(S)]
        out = fl.if2(model.descriptor(), datas, np.zeros(len(th)), 0.5, 1, seeds_of(S), theta0=np.repeat(th[None], S, axis=0), want_last=True)
    assert not out["rc"].any()
    np.testing.assert_array_equal(out["ll"][:, 0], ll)
    for k in range(S):
        np.testing.assert_array_equal(out["ll_t"][k], ll_t[k]); np.testing.assert_array_equal(out["ess_t"][k], ess_t[k])
        np.testing.assert_array_equal(out["anc"][k], ancs[k]); np.testing.assert_array_equal(out["x"][k][:, out["anc"][k]], parts[k])
        np.testing.assert_array_equal(out["theta_mean"][k, 0], th)


def test_the_split_over_launches_and_a_continued_search_change_no_bit():
    model, datas = model_and_series("c2")
    S, n, iters = len(datas), 257, 4
    th = H.theta_of(model)
    theta0 = np.repeat(th[None], S, axis=0)
    sd = np.full(len(th), 0.03)
    with NativePfFleet(model, n, S) as fl:
        run = lambda **kw: fl.if2(model.descriptor(), datas, sd, 0.4, kw.pop("iters", iters), seeds_of(S), want_swarm=True, want_last=True, **kw)
        whole = run(theta0=theta0)
        for per in (2, 3, 1):                                   # 2 + 2, 3 + 1, 1 + 1 + 1 + 1 iterations per launch
            got = run(theta0=theta0, iters_per_launch=per)
            for key in ("theta_mean", "ll", "swarm", "x", "anc", "rc"):
                np.testing.assert_array_equal(got[key], whole[key], err_msg=f"{key}, {per} per launch")
        first = run(theta0=theta0, iters=1)                     # 1 + 3 as two calls: the second continues from the returned swarm
        rest = run(swarm0=first["swarm"], first_iter=1, iters=3)
        np.testing.assert_array_equal(np.concatenate([first["theta_mean"], rest["theta_mean"]], axis=1), whole["theta_mean"])
        np.testing.assert_array_equal(np.concatenate([first["ll"], rest["ll"]], axis=1), whole["ll"])
        for key in ("swarm", "x", "anc"):
            np.testing.assert_array_equal(rest[key], whole[key], err_msg=key)


def test_the_fleet_is_only_lent():
    model, datas = model_and_series("c2")
    datas = [d for d in datas if len(d[0])]
    S, n = len(datas), 100
    th = H.theta_of(model)
    head = [tuple(a[:4] for a in d) for d in datas]
    tail = [tuple(a[4:] for a in d) for d in datas]
    with NativePfFleet(model, n, S) as lent, NativePfFleet(model, n, S) as kept:
        for fl in (lent, kept):
            fl.reseed(seeds_of(S))
            assert not fl.ll_filter(head)[3].any()
        before = [(lent.particles(k), lent.ancestors(k), lent.observation_index(k)) for k in range(S)]
        out = lent.if2(model.descriptor(), datas, np.full(len(th), 0.05), 0.5, 2, [7] * S, theta0=np.repeat(th[None] + 0.3, S, axis=0))
        assert not out["rc"].any()
        for k in range(S):
            np.testing.assert_array_equal(lent.particles(k), before[k][0]); np.testing.assert_array_equal(lent.ancestors(k), before[k][1])
            assert lent.observation_index(k) == before[k][2] == 4
        a, b = lent.ll_filter_more(tail), kept.ll_filter_more(tail)   # ll, clock and parameters: the continued filter is the undisturbed one
        np.testing.assert_array_equal(a[0], b[0])
        for k in range(S):
            np.testing.assert_array_equal(a[1][k], b[1][k]); np.testing.assert_array_equal(a[2][k], b[2][k])
            np.testing.assert_array_equal(lent.particles(k), kept.particles(k))


def test_one_failing_series_has_its_own_status_and_the_others_are_what_they_were():
    model, datas = model_and_series("linear")
    S, n, iters = len(datas), 100, 3
    th = H.theta_of(model)
    theta0 = np.repeat(th[None], S, axis=0)
    sd = np.array([0.05, 0.0, 0.0, 0.05])
    bad = [tuple(a.copy() for a in d) for d in datas]
    bad[3][1][5] = 1e200                                        # every particle's squared residual overflows: no usable weight
    with NativePfFleet(model, n, S) as fl:
        good = fl.if2(model.descriptor(), datas, sd, 0.5, iters, seeds_of(S), theta0=theta0, want_swarm=True, want_last=True)
        got = fl.if2(model.descriptor(), bad, sd, 0.5, iters, seeds_of(S), theta0=theta0, want_swarm=True, want_last=True)
    assert list(good["rc"]) == [0] * S and list(got["rc"]) == [0, 0, 0, _abi.CSSM_ENONFINITE, 0]
    assert np.isnan(got["theta_mean"][3]).all() and np.isnan(got["ll"][3]).all() and np.isnan(got["x"][3]).all()
    assert np.isnan(got["ll_t"][3]).all() and (got["ess_t"][3] == -1).all() and (got["anc"][3] == 0xffffffff).all()
    np.testing.assert_array_equal(got["swarm"][3], np.repeat(th[:, None], n, axis=1))      # the swarm the failing iteration started from
    for k in (0, 1, 2, 4):
        for key in ("theta_mean", "ll", "swarm", "x", "anc"):
            np.testing.assert_array_equal(got[key][k], good[key][k], err_msg=f"{key} of series {k}")
    want = H.twin_search(model, n, bad[3], sd, 0.5, iters, seeds_of(S)[3], theta0=th)
    assert want["rc"] == _abi.CSSM_ENONFINITE


def test_what_needs_a_fleet_to_be_refused():
    lin, c2 = cases.linear_model(), cases.c2_model()
    datas = [(np.arange(3.0), np.ones(3), None)] * 2
    with NativeLgcpFleet(cases.c4_model(), 64, 2, 2) as fl:     # an LGCP fleet, by name
        fl.n_theta = 4                                          # (the Python side checks the row length against the fleet's own model)
        with pytest.raises(CssmError, match="cssm_fleet_if2: an LGCP fleet filters event streams") as e:
            fl.if2(lin.descriptor(), datas, np.zeros(4), 0.5, 1, [1, 2], theta0=np.zeros((2, 4)))
        assert e.value.code == _abi.CSSM_EINVAL_ARG
    with NativePfFleet(c2, 64, 2) as fl:
        fl.n_theta = 4
        with pytest.raises(CssmError, match="not of the fleet's model structure") as e:
            fl.if2(lin.descriptor(), datas, np.zeros(4), 0.5, 1, [1, 2], theta0=np.zeros((2, 4)))
        assert e.value.code == _abi.CSSM_EINVAL_DESC
        fl.n_theta = 10
        lib = load_library()
        off = np.array([0, 3, 2], dtype=np.uint64)
        p = lambda a, ty: a.ctypes.data_as(C.POINTER(ty))
        z, sd, seeds, rc = np.zeros(40), np.zeros(10), np.zeros(2, dtype=np.uint64), np.zeros(2, dtype=np.int32)
        got = lib.cssm_fleet_if2(fl._h, c2.descriptor().ptr(), p(z, C.c_double), None, 10, p(sd, C.c_double), 0.5, 0, 1, 0, p(seeds, C.c_uint64),
                                 p(off, C.c_uint64), p(z, C.c_double), p(z, C.c_double), None, p(z, C.c_double), p(z, C.c_double), None, None, None,
                                 None, None, p(rc, C.c_int))
        assert got == _abi.CSSM_EINVAL_ARG and b"off must be non-decreasing" in lib.cssm_last_error()
        with pytest.raises(CssmError, match="no search has run"):
            fl.if2_last_ms()


def test_the_acceptance_configuration_on_the_device_is_the_twins():
    """The four searches of tests/test_fleet_if2_host.py (N = 300, M = 40, T = 60) in one launch: bit for bit the twin, whose final means
    that file accepts (2 dl <= 5.99) -- and the criterion is evaluated on the device's means here as well."""
    S = len(H.ACC_STARTS)
    model = cases.linear_model()
    theta0 = np.array([H.acc_theta(s) for s in H.ACC_STARTS])
    with NativePfFleet(model, H.ACC_N, S) as fl:
        out = fl.if2(model.descriptor(), [H.acc_data()] * S, H.ACC_SD, H.ACC_COOL, H.ACC_M, H.ACC_SEEDS, theta0=theta0, want_swarm=True)
    assert not out["rc"].any()
    for k in range(S):
        want = H.acc_twin(k)
        np.testing.assert_array_equal(out["theta_mean"][k], want["theta_mean"]); np.testing.assert_array_equal(out["ll"][k], want["ll"])
        np.testing.assert_array_equal(out["swarm"][k], want["swarm"])
        found = H.two_delta(out["theta_mean"][k, -1][list(H.ACC_FREE)])
        print(f"    search {k}: 2dl = {found:.3f}")
        assert found <= H.CHI2_95_2DOF
