"""cssm_pf_if2 (include/cssm_pf.h; an EXTENSION): iterated filtering with ONE swarm of any size, its particles tiled over many workgroups
(cssm_if2.hip).  The contract's section (include/cssm_numerics.h, "iterated filtering") states a search so that nothing depends on how
particles are mapped to lanes or blocks, so every comparison here is bit for bit:

  * against a one-series cssm_fleet_if2 up to its N = 4096, and against the sequential twin (tests/cpp/if2_twin.c through
    tests/test_fleet_if2_host.py::twin_search) beyond -- at the tile edges, at every latent dimension, for every served observation kind;
  * a frozen swarm is cssm_pf_ll_filter under the iteration's key, which ties the path to the filter without the twin;
  * weights that collapse onto one or two particles of one tile; a continued search; a dead search; the handle is only lent; what a
    live handle is refused for;
  * the acceptance configuration of the host file at N = 8192.  The twin's own figures at this size, computed on the CPU: 2 dl of the four
    final means 0.023, 0.022, 0.006, 0.091 (accepted; the threshold is 5.99), of the starting points 78, 17, 57, 173 and of a blind swarm
    (has_obs = 0) 79, 17, 57, 167 (rejected)."""
import ctypes as C

import numpy as np
import pytest

import cases
import test_fleet_if2_host as H
from composablestatespacemodels_amd import CssmError, _abi, load_library
from composablestatespacemodels_amd.filter import NativePf, NativePfFleet

pytestmark = pytest.mark.gpu
SEED = cases.SEED
TILE = _abi.IF2_TILE
CSSM_OPT_RESAMPLER = 2                                          # include/cssm_pf.h
KEYS = ("theta_mean", "ll", "swarm", "ll_t", "ess_t", "x", "anc")


def single(model, n, data, sd, cool, iters, seed, pf=None, **kw):
    """One search on a handle of its own (or on ``pf``), every output asked for."""
    if pf is not None:
        return pf.if2(*data, sd, cool, iters, seed, want_swarm=True, want_last=True, **kw)
    with NativePf(model, n) as own:
        out = own.if2(*data, sd, cool, iters, seed, want_swarm=True, want_last=True, **kw)
        assert own.if2_last_ms() > 0.0 or len(data[0]) == 0
    return out


def assert_same(got, want, what=""):
    assert got["rc"] == want["rc"], (what, got["rc"], want["rc"])
    for key in KEYS:
        np.testing.assert_array_equal(got[key], want[key], err_msg=f"{key} {what}")


def some_sd(model):
    """Every slot walks but one; the scale, where the kind has one, is free."""
    lay = H.layout_of(model)
    nt, scale = int(lay[1]), int(lay[4])
    sd = np.full(nt, 0.02)
    fixed = nt // 2 if nt // 2 != scale else nt // 2 + 1
    if fixed < nt:
        sd[fixed] = 0.0
    return sd


# 1 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["c2", "linear"])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 257, 1000, 4096])
def test_up_to_the_fleets_size_it_is_a_one_series_fleet_search(name, n):
    model, data = H.ragged(name, 9)                             # ragged in dt (a repeated time), an unobserved record
    th, sd, seed = H.theta_of(model) + 0.01, some_sd(model), SEED + 5
    with NativePfFleet(model, n, 1) as fl:
        f = fl.if2(model.descriptor(), [data], sd, 0.5, 3, [seed], theta0=th[None], want_swarm=True, want_last=True)
    want = {"rc": int(f["rc"][0]), **{k: f[k][0] for k in KEYS}}
    got = single(model, n, data, sd, 0.5, 3, seed, theta0=th)
    assert got["rc"] == 0 and np.isfinite(got["theta_mean"]).all()
    assert_same(got, want, f"{name} N = {n}")


# 2 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [4097, 8192, 2 * TILE, 2 * TILE + 1, 3 * TILE - 1, 65537])
def test_beyond_the_fleet_it_is_the_twin(n):
    model, data = H.ragged("c2", 6)
    th, sd, seed = H.theta_of(model) - 0.01, some_sd(model), SEED + 6
    got = single(model, n, data, sd, 0.5, 2, seed, theta0=th)
    assert got["rc"] == 0 and np.isfinite(got["theta_mean"]).all()
    assert_same(got, H.twin_search(model, n, data, sd, 0.5, 2, seed, theta0=th), f"N = {n}")


# 3 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", list(range(1, 17)))
def test_every_latent_dimension(d):
    """k_if2_start<D> and k_if2_weigh<D> for every D, the models of tests/test_gpu_fleet_if2.py::test_every_latent_dimension."""
    model = cases.dim_model(d)
    t, y, has = cases.poisson_counts(4)
    has = has.copy(); has[2] = 0
    th = H.theta_of(model) - 0.02
    sd = np.full(len(th), 0.03)
    got = single(model, 4099, (t, y, has), sd, 0.5, 2, SEED + d, theta0=th)
    assert got["rc"] == 0
    assert_same(got, H.twin_search(model, 4099, (t, y, has), sd, 0.5, 2, SEED + d, theta0=th), f"d = {d}")


# 4 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", H.FROZEN)
def test_every_served_observation_model(name):
    model, data = H.ragged(name)
    th, sd = H.theta_of(model), some_sd(model)
    got = single(model, 5000, data, sd, 0.5, 2, SEED + 7, theta0=th)
    assert got["rc"] == 0
    assert_same(got, H.twin_search(model, 5000, data, sd, 0.5, 2, SEED + 7, theta0=th), name)


# 5 ------------------------------------------------------------------------------------------------------------------------------
def test_a_frozen_swarm_is_the_plain_filter_under_the_iteration_key():
    model, data = H.ragged("c2", 9)
    n, seed = 65539, SEED + 8
    th = H.theta_of(model)
    with NativePf(model, n, seed=int(load_library().cssm_pf_run_key(seed, 1))) as pf:
        ll, ll_t, ess_t, _ = pf.run(*data)
        prop, anc = pf.proposed(), pf.ancestors()
    got = single(model, n, data, np.zeros(len(th)), 0.5, 1, seed, theta0=th)
    assert got["rc"] == 0 and got["ll"][0] == ll
    np.testing.assert_array_equal(got["ll_t"], ll_t); np.testing.assert_array_equal(got["ess_t"], ess_t)
    np.testing.assert_array_equal(got["x"], prop); np.testing.assert_array_equal(got["anc"], anc)
    np.testing.assert_array_equal(got["swarm"], np.repeat(th[:, None], n, axis=1)); np.testing.assert_array_equal(got["theta_mean"][0], th)


# 6 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [12289, 65537])
def test_collapsed_weights_across_tiles(n):
    """An outlying observation at record 4 leaves a handful of particles with all the weight: an owner of (almost) every slot of every
    tile.  The twin's ESS at that record in the last iteration, computed on the CPU with these settings: 7 (N = 12 289) and 3 (65 537) over
    nine records, 3 and 2 over the first five."""
    model = cases.linear_model()
    t, y, has = cases.gaussian_series(9)
    y = y.copy(); y[4] += 6.0
    th = H.theta_of(model)
    for T in (9, 5):                                            # all records; then up to the collapsed one, whose ancestors anc_out are
        data = (t[:T], y[:T], has[:T])
        want = H.twin_search(model, n, data, H.ACC_SD, 0.5, 2, SEED + 9, theta0=th)
        assert want["rc"] == 0 and 1 <= want["ess_t"][4] <= 16, want["ess_t"]   # fewer effective particles than a quarter of a wave holds
        got = single(model, n, data, H.ACC_SD, 0.5, 2, SEED + 9, theta0=th)
        assert_same(got, want, f"N = {n}, T = {T}")
        if T == 5:
            assert len(np.unique(got["anc"])) < n // 64         # the slots belong to a handful of particles


# 7 ------------------------------------------------------------------------------------------------------------------------------
def test_a_search_continued_from_its_swarm_is_the_uninterrupted_one():
    model, data = H.ragged("c2", 8)
    n, seed = 4097, SEED + 10
    th, sd = H.theta_of(model), some_sd(model)
    with NativePf(model, n) as pf:
        whole = single(model, n, data, sd, 0.4, 4, seed, pf=pf, theta0=th)
        first = single(model, n, data, sd, 0.4, 1, seed, pf=pf, theta0=th)
        rest = single(model, n, data, sd, 0.4, 3, seed, pf=pf, swarm0=first["swarm"], first_iter=1)
    np.testing.assert_array_equal(np.vstack([first["theta_mean"], rest["theta_mean"]]), whole["theta_mean"])
    np.testing.assert_array_equal(np.concatenate([first["ll"], rest["ll"]]), whole["ll"])
    for key in ("swarm", "ll_t", "ess_t", "x", "anc"):
        np.testing.assert_array_equal(rest[key], whole[key], err_msg=key)


# 8 ------------------------------------------------------------------------------------------------------------------------------
def dead_in_the_second_iteration():
    """y[5] = 1e200: the squared residual overflows for every observation sd below 1e46.  Iteration 0 walks the log sd with a standard
    deviation of 60 per perturbation, so some particles stand beyond log(1e46) = 106 at record 5 and the search lives; the records behind
    it bring the swarm back, iteration 1 walks by 60 * (1e-300)^(1/50) = 6e-5, and at record 5 no particle has a usable weight."""
    model = cases.linear_model()
    t, y, has = cases.gaussian_series(9)
    bad = y.copy(); bad[5] = 1e200
    return model, (t, y, has), (t, bad, has), np.array([60.0, 0.0, 0.0, 0.0]), 1e-300


def test_a_dead_search_is_a_status_and_the_handle_filters_as_before():
    model, good, bad, sd, cool = dead_in_the_second_iteration()
    n, seed = 4097, SEED + 11
    th = H.theta_of(model)
    want = H.twin_search(model, n, bad, sd, cool, 3, seed, theta0=th)
    assert want["rc"] == _abi.CSSM_ENONFINITE and np.isfinite(want["theta_mean"][0]).all() and np.isnan(want["theta_mean"][1:]).all()
    with NativePf(model, n) as pf:
        before = pf.run(*good)[:3] + (pf.particles(), pf.ancestors())
        got = single(model, n, bad, sd, cool, 3, seed, pf=pf, theta0=th)
        after = pf.run(*good)[:3] + (pf.particles(), pf.ancestors())
    assert got["rc"] == _abi.CSSM_ENONFINITE
    assert_same(got, want)                                      # rows from the failing iteration on NaN; the swarm that iteration started from
    assert np.isnan(got["ll"][1:]).all() and np.isfinite(got["ll"][0]) and not np.array_equal(got["swarm"], np.repeat(th[:, None], n, axis=1))
    assert np.isnan(got["ll_t"]).all() and (got["ess_t"] == -1).all() and np.isnan(got["x"]).all() and (got["anc"] == 0xffffffff).all()
    for a, b in zip(before, after):
        np.testing.assert_array_equal(a, b)


# 9 ------------------------------------------------------------------------------------------------------------------------------
def test_the_handle_is_only_lent():
    model, (t, y, has) = H.ragged("c2", 9)
    n = 5000
    th, sd = H.theta_of(model), some_sd(model)

    def sequence(lend):
        rows = []
        with NativePf(model, n, seed=SEED + 12) as pf:
            pf.init(float(t.min()))
            for s in range(4):
                rows.append(pf.step(t[s], y[s], bool(has[s])))
            if lend:
                out = pf.if2(t, y, has, sd, 0.5, 2, 77, theta0=th + 0.3)
                assert out["rc"] == 0 and np.isfinite(out["theta_mean"]).all()
                rows.append((pf.particles(), pf.ancestors()))
            else:
                rows.append((pf.particles(), pf.ancestors()))
            for s in range(4, 9):
                rows.append(pf.step(t[s], y[s], bool(has[s])))
            rows.append((pf.particles(), pf.ancestors()))
        return rows

    for a, b in zip(sequence(True), sequence(False)):
        for u, v in zip(a, b):
            np.testing.assert_array_equal(u, v)


# 10 -----------------------------------------------------------------------------------------------------------------------------
def _refused(pf, data, nt, code, words):
    with pytest.raises(CssmError) as e:
        pf.if2(*data, np.zeros(nt), 0.5, 1, 1, theta0=np.zeros(nt))
    assert e.value.code == code, e.value
    for w in words:
        assert w in str(e.value), (w, str(e.value))


def test_what_a_live_handle_is_refused_for():
    c2, data = H.ragged("c2", 6)
    with NativePf(cases.c4_model(), 1000, lgcp_precision=2) as pf:                        # an LGCP handle, by name
        ev = cases.event_times(6)
        before = pf.run(*ev)[:3]
        _refused(pf, ev, 5, _abi.CSSM_EINVAL_ARG, ("cssm_pf_if2", "LGCP handle is not served"))
        for a, b in zip(before, pf.run(*ev)[:3]):
            np.testing.assert_array_equal(a, b)
    with NativePf(c2, 1000) as pf:
        before = pf.run(*data)[:3]
        _refused(pf, data, 9, _abi.CSSM_EINVAL_ARG, ("n_theta = 9", "flattens to 10"))     # a wrong n_theta
        pf.set_option(CSSM_OPT_RESAMPLER, 1)                                          # a stratified handle, naming the option
        _refused(pf, data, 10, _abi.CSSM_ESTATE, ("CSSM_OPT_RESAMPLER", "systematic"))
        pf.set_option(CSSM_OPT_RESAMPLER, 0)
        for a, b in zip(before, pf.run(*data)[:3]):
            np.testing.assert_array_equal(a, b)
        with pytest.raises(CssmError, match="no search has run"):
            pf.if2_last_ms()
        assert pf.if2(*data, np.zeros(10), 0.5, 1, 1, theta0=H.theta_of(c2))["rc"] == 0    # ... and is served once it is systematic again

    class Shard:                                                                           # the only shard of a cloud of 1000 (test_gpu_smooth.py)
        lib = load_library()
        _h = C.c_void_p()

    _abi.check(Shard.lib.cssm_pf_create_shard(c2.descriptor().ptr(), 1000, 0, 1000, 7, 0, None, C.byref(Shard._h)))
    try:
        pf = NativePf.__new__(NativePf)
        pf.lib, pf._h, pf.n, pf.d, pf.generation = Shard.lib, Shard._h, 1000, 3, 0
        try:
            _refused(pf, data, 10, _abi.CSSM_ESTATE, ("cssm_pf_if2 runs on a single-GPU handle",))
        finally:
            pf._h = C.c_void_p()                                                           # (Shard owns the handle)
    finally:
        Shard.lib.cssm_pf_destroy(Shard._h)


# 11 -----------------------------------------------------------------------------------------------------------------------------
ACC_N = 8192


@pytest.mark.parametrize("k", range(len(H.ACC_STARTS)))
def test_truth(k):
    """The acceptance configuration of tests/test_fleet_if2_host.py (T = 60, 40 iterations, cooling 0.25) at N = 8192: equal to the twin,
    the final mean inside the 95 % likelihood-ratio region, the starting point and a swarm that only random-walks outside it."""
    model = cases.linear_model()
    t, y, has = H.acc_data()
    th = H.acc_theta(H.ACC_STARTS[k])
    got = single(model, ACC_N, (t, y, has), H.ACC_SD, H.ACC_COOL, H.ACC_M, H.ACC_SEEDS[k], theta0=th)
    want = H.twin_search(model, ACC_N, (t, y, has), H.ACC_SD, H.ACC_COOL, H.ACC_M, H.ACC_SEEDS[k], theta0=th)
    assert got["rc"] == 0
    assert_same(got, want, f"search {k}")
    found = H.two_delta(got["theta_mean"][-1][list(H.ACC_FREE)])
    start = H.two_delta(H.ACC_STARTS[k])
    blind = H.twin_search(model, ACC_N, (t, y, np.zeros_like(has)), H.ACC_SD, H.ACC_COOL, H.ACC_M, H.ACC_SEEDS[k], theta0=th)
    walk = H.two_delta(blind["theta_mean"][-1][list(H.ACC_FREE)])
    print(f"    search {k}: start 2dl = {start:.2f}; 2dl = {found:.3f}; has_obs = 0: 2dl = {walk:.2f}")
    assert found <= H.CHI2_95_2DOF, (k, found)
    assert start > H.CHI2_95_2DOF, (k, start)
    assert walk > H.CHI2_95_2DOF, (k, walk)
