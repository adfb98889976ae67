"""cssm_pf_smooth (include/cssm_pf.h; an EXTENSION): forward filtering, backward simulation on ONE handle, the slots of the cloud tiled
over many workgroups (csrc/cssm_smooth.hip).  Two references, both bit for bit:

  * N <= CSSM_FLEET_MAX_N: series 0 of a one-series fleet under the same key (cssm_fleet_smooth, whose kernel keeps the cloud in one
    workgroup) -- ll, trajectories and every order statistic ==, the means (the same plain fp64 sums) within rtol 1e-12, atol 0;
  * any N: the sequential twin of the contract's backward simulation (tests/cpp/backsim_twin.c) on the ORACLE's history -- trajectories
    and ll ==.

CSSM_OPT_SMOOTH_TILE puts many tiles under a small cloud; the results may not depend on it."""
import ctypes as C

import numpy as np
import pytest

import cases
from composablestatespacemodels_amd import CssmError, _abi
from composablestatespacemodels_amd.filter import NativePf, NativePfFleet
from oracle import oracle
from test_fleet_smooth_host import kinds_of, oracle_history, pack_records, rank_truth, twin_traj
from test_gpu_fleet import _GEN, ragged_c2
from test_smooth_host import PREMISE_M, PREMISE_N, PREMISE_R, PREMISE_SEED0, premise_case, premise_twin

pytestmark = pytest.mark.gpu
SEED = cases.SEED
TILE = _abi.SMOOTH_TILE
OPT_TILE = _abi.CSSM_OPT_SMOOTH_TILE


def c2_series(T=12):
    """One C2 series of ragged_c2 (dt = 0.5, an origin of its own), with observations removed and a repeated time (dt = 0) in it"""
    models, seeds, datas = ragged_c2(2)
    t, y, has = datas[1]
    assert len(t) == 12
    t, y, has = t[:T].copy(), y[:T].copy(), has[:T].copy()
    has[2] = 0
    if T > 7:
        has[7] = 0
    t[4] = t[3]; has[4] = 1
    return models[1], seeds[1], (t, y, has)


def handle_smooth(model, n, key, data, M, tile=None, resampler=None):
    """(ll, mean, lower, upper, eta_of_mean, eta_lower, eta_upper, traj) of a fresh handle"""
    with NativePf(model, n, key) as g:
        if tile is not None:
            g.set_option(OPT_TILE, tile)
        if resampler is not None:
            g.set_option(2, resampler)                         # CSSM_OPT_RESAMPLER
        return g.smooth(*data, n_traj=M, want_trajectories=True)


def fleet_smooth(model, n, key, data, M):
    """the same tuple from series 0 of a one-series fleet"""
    with NativePfFleet(model, n, 1) as fl:
        fl.reseed([key])
        ll, rows, rc, traj = fl.smooth([data], n_traj=M, want_trajectories=True)
    assert not rc.any(), rc
    return (ll[0],) + tuple(rows[0]) + (traj[0],)


def assert_equals_fleet(got, want):
    assert got[0] == want[0], (got[0], want[0])
    np.testing.assert_array_equal(got[7], want[7])
    for q in (2, 3, 5, 6):
        np.testing.assert_array_equal(got[q], want[q])
    for q in (1, 4):
        np.testing.assert_allclose(got[q], want[q], rtol=1e-12, atol=0)      # plain fp64 sums
    assert np.all(np.isfinite(got[1])) and np.all(np.isfinite(got[6]))


def assert_same_bits(a, b):
    assert a[0] == b[0]
    for x, y in zip(a[1:], b[1:]):
        np.testing.assert_array_equal(x, y)


def twin_of(model, n, key, data, M, flags=0):
    """(ll, traj) of the oracle's forward pass (under the oracle's resampler flag) and the twin's backward simulation"""
    t, y, has = data
    if flags == 0:
        ll, X, Anc = oracle_history(model, n, key, data)
    else:
        o = oracle.OraclePf(model.descriptor(), n, key, flags)
        o.init(float(np.min(t)))
        X, Anc, ll = [o.particles()], [o.ancestors()], 0.0
        for s in range(len(t)):
            ll, _ = o.step(float(t[s]), float(y[s]), bool(has[s]))
            X.append(o.proposed()); Anc.append(o.ancestors())
        X, Anc = np.array(X), np.array(Anc)
    return ll, twin_traj(X, Anc, pack_records(model, n, key, t, y, has), kinds_of(model), key, M), X, Anc


# 1 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,M", [(1, 1), (2, 63), (63, 64), (64, 65), (65, 200), (129, 1), (1000, 63), (_abi.FLEET_MAX_N, 200)])
def test_against_the_fleet_under_every_tile_setting(n, M):
    model, key, data = c2_series()
    want = fleet_smooth(model, n, key, data, M)
    got = [handle_smooth(model, n, key, data, M, tile) for tile in (64, 128, None)]
    assert got[0][7].shape == (len(data[0]) + 1, M) and got[0][1].shape == (len(data[0]) + 1, 3)
    assert_equals_fleet(got[0], want)
    assert_same_bits(got[1], got[0])
    assert_same_bits(got[2], got[0])


# 2 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [_abi.FLEET_MAX_N + 1, 2 * TILE, 2 * TILE + 1, 3 * TILE - 1])
def test_against_the_twin_at_the_default_tile(n):
    model, key, data = c2_series(6)
    M = 70
    ll, traj, _, _ = twin_of(model, n, key, data, M)
    got = handle_smooth(model, n, key, data, M)
    assert got[0] == ll, (got[0], ll)
    np.testing.assert_array_equal(got[7], traj)
    assert np.all(np.isfinite(got[1])) and np.all(got[2] <= got[3])


# 3 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", list(range(1, 17)))
def test_every_latent_dimension(d):
    """One instantiation of each of the kernels per latent dimension (tests/test_smooth_host.py holds this list to the source)."""
    model = cases.dim_model(d)
    t, y, has = cases.poisson_counts(6, seed=SEED + d)
    has = has.copy(); has[2] = 0
    with NativePf(model, 257, SEED + 17) as g:
        assert g.d == d
        g.set_option(OPT_TILE, 64)
        got = g.smooth(t, y, has, n_traj=70, want_trajectories=True)
    assert_equals_fleet(got, fleet_smooth(model, 257, SEED + 17, (t, y, has), 70))


# 4 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in cases.GOLDEN_NAMES if n != "c4"] + ["gbsg", "euler"])
def test_every_served_observation_model(name):
    model = cases.literal_case(name, 12)[0]
    data = _GEN[name](12, seed=SEED + 3)
    got = handle_smooth(model, 1000, SEED + 34, data, 100, tile=256)
    assert_equals_fleet(got, fleet_smooth(model, 1000, SEED + 34, data, 100))


# 5 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,flag", [(1, oracle.RESAMPLE_STRATIFIED), (2, oracle.RESAMPLE_MULTINOMIAL)])
def test_the_other_resamplers_against_the_twin(kind, flag):
    """Backward simulation reads only clouds and ancestors: multinomial's unsorted ancestors are served like any others."""
    model, key, data = c2_series()
    n, M = 1000, 100
    ll, traj, _, Anc = twin_of(model, n, key, data, M, flags=flag)
    if kind == 2:
        assert any(np.any(np.diff(a.astype(np.int64)) < 0) for a in Anc)       # (the premise: they are not sorted)
    got = handle_smooth(model, n, key, data, M, tile=256, resampler=kind)
    assert got[0] == ll, (got[0], ll)
    np.testing.assert_array_equal(got[7], traj)


# 6 ------------------------------------------------------------------------------------------------------------------------------
def _genealogy(Anc, n, M):
    T = len(Anc) - 1
    want = np.zeros((T + 1, M), dtype=np.uint32)
    want[T] = Anc[T][(np.arange(M, dtype=np.uint64) * np.uint64(n) // np.uint64(M)).astype(np.int64)]
    for s in range(T - 1, -1, -1):
        want[s] = Anc[s][want[s + 1]]
    return want


def test_records_without_a_density_follow_the_ancestors():
    n, M = 1000, 100
    # every record at one time: dt = 0 throughout
    model, key, (t, y, has) = c2_series(6)
    t = np.full(6, t[0])
    _, _, Anc = oracle_history(model, n, key, (t, y, has))
    got = handle_smooth(model, n, key, (t, y, has), M, tile=256)
    np.testing.assert_array_equal(got[7], _genealogy(Anc, n, M))
    # a Brownian component with zero diffusion: sd = 0 at every dt
    from composablestatespacemodels_amd import Model, Parameters, Sde
    from composablestatespacemodels_amd.model import BrownianParameter
    frozen = Model.linear(Sde.brownianMotion(1)).run(Parameters.apply(np.log(0.5), BrownianParameter([0.5], [np.log(2.0)], [-np.inf])))
    data = cases.gaussian_series(6)
    recs = pack_records(frozen, n, key, *data).reshape(6, 80 + 40)
    assert all(np.frombuffer(r[80:112].tobytes())[3] == 0.0 for r in recs) and np.frombuffer(recs[1][56:64].tobytes())[0] > 0.0
    ll, X, Anc = oracle_history(frozen, n, key, data)
    got = handle_smooth(frozen, n, key, data, M, tile=256)
    assert got[0] == ll
    np.testing.assert_array_equal(got[7], _genealogy(Anc, n, M))


def test_an_unweighted_last_record_starts_from_the_identity():
    model, key, (t, y, has) = c2_series()
    has = has.copy(); has[-1] = 0
    n, M = 1000, 63
    got = handle_smooth(model, n, key, (t, y, has), M, tile=256)
    np.testing.assert_array_equal(got[7][-1], (np.arange(M) * n) // M)
    ll, traj, _, _ = twin_of(model, n, key, (t, y, has), M)
    assert got[0] == ll
    np.testing.assert_array_equal(got[7], traj)


# 7 ------------------------------------------------------------------------------------------------------------------------------
def _raw(g, data, n_traj=10, interval=0.975, flags=0):
    t, y, has = (np.ascontiguousarray(a) for a in data)
    p = lambda a, ty: a.ctypes.data_as(C.POINTER(ty))
    ll = C.c_double(7.0)
    rc = g.lib.cssm_pf_smooth(g._h, p(t, C.c_double), p(y, C.c_double), p(has.astype(np.uint8), C.c_uint8), len(t), n_traj, interval, flags,
                              C.byref(ll), *([None] * 6), None)
    return rc, g.lib.cssm_last_error(), ll.value


def test_refusals_leave_a_handle_that_filters_as_before():
    model, key, data = c2_series()
    n = 1000
    with NativePf(model, n, key) as fresh:
        want = fresh.run(*data)
        want_cloud = fresh.particles()
    with NativePf(model, n, key) as g:
        with pytest.raises(CssmError) as e:
            g.smooth_last_ms()
        assert e.value.code == _abi.CSSM_ESTATE

        def still_filters():
            got = g.run(*data)
            assert got[0] == want[0]
            np.testing.assert_array_equal(got[1], want[1]); np.testing.assert_array_equal(got[2], want[2])
            np.testing.assert_array_equal(g.particles(), want_cloud)

        for kw, word in (({"n_traj": 0}, b"n_traj must be in [1, CSSM_FLEET_MAX_N = 4096]"), ({"n_traj": _abi.FLEET_MAX_N + 1}, b"(got 4097)"),
                         ({"flags": 1}, b"CSSM_INTERP_REFERENCE_PAIRING is not offered"), ({"flags": 2}, b"unknown flag bits 0x2"),
                         ({"interval": 0.0}, b"interval must be in (0, 1]"), ({"interval": 1.5}, b"interval must be in (0, 1]")):
            rc, msg, ll = _raw(g, data, **kw)
            assert rc == _abi.CSSM_EINVAL_ARG and word in msg and ll == 7.0, (kw, rc, msg)
            still_filters()
        for bad in (65, 1, 63, -64):
            with pytest.raises(CssmError) as e:
                g.set_option(OPT_TILE, bad)
            assert e.value.code == _abi.CSSM_EINVAL_ARG and "multiple of 64" in str(e.value)
        still_filters()
        with pytest.raises(CssmError) as e:                     # no refusal counted as a call
            g.smooth_last_ms()
        assert e.value.code == _abi.CSSM_ESTATE
        # a call, then the handle filters like a fresh one once it is initialised again
        out = g.smooth(*data, n_traj=64)
        assert out[0] == want[0]
        ms = g.smooth_last_ms()
        assert len(ms) == 3 and all(v >= 0.0 for v in ms)
        with pytest.raises(CssmError) as e:                     # its own buffers hold no cloud now
            g.step(float(data[0][-1]) + 1.0, 1.0)
        assert e.value.code == _abi.CSSM_ESTATE
        still_filters()
    with NativePfFleet(model, n, 1) as fl:                      # a fleet keeps refusing the option
        with pytest.raises(CssmError) as e:
            fl.set_option(OPT_TILE, 64)
        assert e.value.code == _abi.CSSM_EINVAL_ARG


def test_an_lgcp_handle_is_refused():
    t, y, has = cases.event_times(5)
    with NativePf(cases.c4_model(), 500, SEED, lgcp_precision=2) as fresh:
        want = fresh.run(t, y, has)
    with NativePf(cases.c4_model(), 500, SEED, lgcp_precision=2) as g:
        rc, msg, _ = _raw(g, (t, y, has))
        assert rc == _abi.CSSM_EINVAL_ARG and b"cssm_pf_smooth: an LGCP handle" in msg and b"chain of sub-steps" in msg
        got = g.run(t, y, has)
        assert got[0] == want[0]
        np.testing.assert_array_equal(got[1], want[1])


def test_a_shard_is_refused():
    """a handle created with the sharded flag (the only shard of a cloud of 1000), on the default stream"""
    model, key, data = c2_series()

    class Shard:
        lib = _abi.load_library()
        _h = C.c_void_p()

    desc = model.descriptor()
    _abi.check(Shard.lib.cssm_pf_create_shard(desc.ptr(), 1000, 0, 1000, key, 0, None, C.byref(Shard._h)))
    try:
        rc, msg, ll = _raw(Shard, data)
        assert rc == _abi.CSSM_ESTATE and b"cssm_pf_smooth runs on a single-GPU handle" in msg and ll == 7.0
    finally:
        Shard.lib.cssm_pf_destroy(Shard._h)


# 8 ------------------------------------------------------------------------------------------------------------------------------
def test_truth():
    """The premise case of tests/test_smooth_host.py on the device: R = 16 calls on one handle, re-keyed between them.  The device equals
    the twin bit for bit, so its z figures are the ones that file's docstring records."""
    import test_grid_smoother as tg
    model, t, y, has = premise_case()
    tr = rank_truth(model, t, y, has, PREMISE_M)
    outs, trajs = [], {}
    with NativePf(model, PREMISE_N, PREMISE_SEED0) as g:
        for r in range(PREMISE_R):
            g.reseed(PREMISE_SEED0 + r)
            out = g.smooth(t, y, has, n_traj=PREMISE_M, want_trajectories=True)
            outs.append(out[:7]); trajs[r] = out[7]
    for r in (0, PREMISE_R - 1):
        ll, traj, rows = premise_twin(r)
        assert outs[r][0] == ll
        np.testing.assert_array_equal(trajs[r], traj)
        for q in (1, 2, 4, 5):
            np.testing.assert_array_equal(outs[r][q + 1], rows[q])
        tg.check_eta_of_mean(model, t, outs[r][1], outs[r][4])
    print(f"\nlinear, T = {len(t)}, N = {PREMISE_N}, n_traj = {PREMISE_M}, R = {PREMISE_R}")
    tg.check_smoothing("cssm_pf_smooth", tg.stack(outs), tr)
