"""-m gpu: SimulateData on the device (include/cssm_pf.h: cssm_simulate, cssm_simulate_from; csrc/cssm_simulate.hip: k_simulate), held
against the oracle's chain bit for bit, built from the existing pieces only, as tests/test_gpu_forecast.py::expected builds a forecast's:

  row 0    = OraclePf(desc, n, key).init(t0): its cloud, its eta(), and the host twin of include/cssm_obs_draws.h on those etas under
             step 0xFFFFFFFF;
  row h    = propagate_only(t_h) / proposed() / set_particles / eta() and the twin's draw under step h - 1.

Then the identities with a handle, the independence of the chunking, every latent dimension, the keys, an exact answer that needs no
oracle (K2 of SURVEY 8c) and the refusals."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import pytest

import cases
from composablestatespacemodels_amd import _abi
from composablestatespacemodels_amd.filter import NativePf
from composablestatespacemodels_amd.model import Model, Parameters, Sde, SdeParameter, logistic
from composablestatespacemodels_amd.simulate import SimulateData, points_of, simulate, simulate_from
from oracle import oracle
from test_forecast_draws import build_twin
from test_gpu_forecast import MODELS, case

pytestmark = pytest.mark.gpu

KEY = 0x51DA7A
BLOCK = 256          # CSSM_BLOCK: pairs per workgroup of k_simulate
ROW0 = 0xFFFFFFFF    # CSSM_SIM_STEP_ROW0
_dp = C.POINTER(C.c_double)


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    return build_twin(tmp_path_factory.mktemp("twin"))


def sim_times(t0):
    return t0 + np.array([0.5, 0.5, 1.75, 3.0, 7.25])   # dt = 0.5, 0 (an equal pair), 1.25, 1.25, 4.25


def expected(model, n, key, t0, times, twin):
    """[T + 1, d + 3, n] with the gamma row left NaN (the oracle states eta = link(gamma), not gamma)."""
    desc = model.descriptor()
    L = desc.leaf_array[0]
    kind, df = desc.desc.obs_kind, desc.desc.obs_df
    o = oracle.OraclePf(desc, n, key)
    o.init(float(t0))
    rows = []

    def row(x, step):
        e = np.ascontiguousarray(o.eta())
        out = np.zeros(n)
        assert twin.twin_obs_draw(kind, e.ctypes.data_as(_dp), n, L.has_scale, L.scale, df, key, step, out.ctypes.data_as(_dp)) == 0
        rows.append(np.vstack([x, np.full((1, n), np.nan), e[None], out[None]]))

    row(o.particles(), ROW0)
    for h, th in enumerate(times):
        o.propagate_only(float(th), None, False)
        x = o.proposed()
        o.set_particles(x)
        row(x, h)
    return np.array(rows)


def assert_rows(got, want):
    d = got.shape[1] - 3
    assert got.shape == want.shape
    assert np.array_equal(got[:, :d], want[:, :d]), "states"
    assert np.array_equal(got[:, d + 1], want[:, d + 1]), "eta"
    assert np.array_equal(got[:, d + 2], want[:, d + 2]), "obs"
    assert np.all(np.isfinite(got[:, d])), "gamma"


@pytest.mark.parametrize("n", [1, 2, 5, 2 * BLOCK + 1])
@pytest.mark.parametrize("name", MODELS)
def test_simulate_matches_the_oracle_chain_bit_for_bit(name, n, twin):
    model = case(name)[0]
    t0 = 1.25
    times = sim_times(t0)
    got = simulate(model, t0, times, n, KEY)
    assert_rows(got, expected(model, n, KEY, t0, times, twin))


@pytest.mark.parametrize("n", [1, 5, 2 * BLOCK + 1, 4100])
def test_rows_are_a_handles_initial_cloud_and_its_forecast_samples(n):
    model = cases.c2_model()
    t0 = 0.5
    times = sim_times(t0)
    got = simulate(model, t0, times, n, KEY)
    with NativePf(model, n, cases.SEED) as g:
        g.reseed(KEY)
        g.init(t0)
        assert np.array_equal(got[0, :g.d], g.particles())
        r = g.forecast(times, KEY, 0.975, want_samples=True)
        assert np.array_equal(got[1:], r["samples"])


@pytest.mark.parametrize("n", [1, 5, 2 * BLOCK + 1])
def test_the_chunking_does_not_show(n):
    model = cases.c3_model()
    times = sim_times(0.0)
    want = simulate(model, 0.0, times, n, KEY)
    for rows in (1, 2, len(times) + 1):
        assert np.array_equal(simulate(model, 0.0, times, n, KEY, rows_per_launch=rows), want, equal_nan=True), rows


@pytest.mark.parametrize("d", range(1, 17))
def test_every_latent_dimension(d, twin):
    model = cases.dim_model(d)
    times = np.array([0.75, 2.0])
    got = simulate(model, 0.0, times, 3, KEY + d)
    assert got.shape == (3, d + 3, 3)
    assert_rows(got, expected(model, 3, KEY + d, 0.0, times, twin))


def test_keys_and_path_identity():
    model = cases.c2_model()
    times = sim_times(0.0)
    a = simulate(model, 0.0, times, 4, KEY)
    assert np.array_equal(a, simulate(model, 0.0, times, 4, KEY))
    b = simulate(model, 0.0, times, 4, KEY + 1)
    assert not np.array_equal(a[:, :3], b[:, :3])
    # path i is a function of (key, i) alone, but for the pairing of the unpaired last path: i < n - 1 of n = 4 within n = 6
    c = simulate(model, 0.0, times, 6, KEY)
    assert np.array_equal(a[:, :, :3], c[:, :, :3])


def test_a_continued_simulation_is_the_one_simulation():
    """cssm_simulate_from: blocks that hand on their last states and count their steps on are one cssm_simulate."""
    model = cases.c2_model()
    times = sim_times(0.0)
    for n in (1, 5):
        whole = simulate(model, 0.0, times, n, KEY)
        head = simulate(model, 0.0, times[:2], n, KEY)
        tail = simulate_from(model, head[-1, :3], 2, float(times[1]), times[2:], KEY)
        assert np.array_equal(head, whole[:3]) and np.array_equal(tail, whole[3:])
    # ... which is how the lazy iterators run: the points do not depend on the block size
    sd = SimulateData(model, seed=7)
    it = sd.simMarkov(0.1, block=4)
    pts = [next(it) for _ in range(11)]
    grid = [p.t for p in pts[1:]]
    want = points_of(0.0, grid, simulate(model, 0.0, grid, 1, sd.key))
    assert [p.t for p in pts] == [p.t for p in want] and pts[0].t == 0.0
    assert all(a.observation == b.observation and a.eta == b.eta and a.gamma == b.gamma and np.array_equal(a.sdeState, b.sdeState)
               for a, b in zip(pts, want))
    got = sd.simPompModel(0.0)(grid)
    assert all(a.observation == b.observation and np.array_equal(a.sdeState, b.sdeState) for a, b in zip(got, want))


def test_known_answer_one_ou_step_from_the_initial_distribution():
    """K2 of SURVEY 8c without the oracle: x0 ~ N(m0, c0), one exact OU step of dt, a Gaussian observation of sd exp(scale).
    mean = mu + (m0 - mu) e^{-phi dt}, var = c0 e^{-2 phi dt} + sigma^2 / (2 phi) (1 - e^{-2 phi dt}), phi the double logistic of the
    given value; the observation adds exp(scale)^2.  Bounds: 5 standard errors, sqrt(var / n) for a mean and var sqrt(2 / (n - 1)) for
    the variance of a Gaussian sample."""
    m0, c0, phi_in, mu, sigma, scale, dt, n = 0.5, 0.8, 0.2, 2.0, 0.7, math.log(0.3), 1.5, 4096
    model = Model.linear(Sde.ouProcess(1)).run(Parameters.apply(scale, SdeParameter.ouParameter(m0, c0, phi_in, mu, sigma)))
    r = simulate(model, 0.0, [dt], n, KEY)
    phi = logistic(logistic(phi_in))
    mean = mu + (m0 - mu) * math.exp(-phi * dt)
    var = c0 * math.exp(-2 * phi * dt) + sigma**2 / (2 * phi) * (1 - math.exp(-2 * phi * dt))
    for name, v, vv in (("state", r[1, 0], var), ("obs", r[1, 3], var + math.exp(scale)**2)):
        print(name, v.mean() - mean, 5 * math.sqrt(vv / n), v.var(ddof=1) - vv, 5 * vv * math.sqrt(2.0 / (n - 1)))
        assert abs(v.mean() - mean) <= 5 * math.sqrt(vv / n), name
        assert abs(v.var(ddof=1) - vv) <= 5 * vv * math.sqrt(2.0 / (n - 1)), name
    # (the row at t0 is the initial distribution itself)
    assert abs(r[0, 0].mean() - m0) <= 5 * math.sqrt(c0 / n) and abs(r[0, 0].var(ddof=1) - c0) <= 5 * c0 * math.sqrt(2.0 / (n - 1))
    assert np.array_equal(r[:, 1], r[:, 0]) and np.array_equal(r[:, 2], r[:, 0])   # gamma = x, eta = gamma for the linear model


def _raw(model, n, t0, times, out):
    lib = _abi.load_library()
    desc = model if hasattr(model, "ptr") else model.descriptor()
    t = None if times is None else np.ascontiguousarray(times, dtype=np.float64)
    return lib.cssm_simulate(desc.ptr(), n, KEY, float(t0), None if t is None else t.ctypes.data_as(_dp), 0 if t is None else len(t), 0, 0,
                             None if out is None else out.ctypes.data_as(_dp)), _abi.last_error()


def test_refusals_name_their_cause_and_write_nothing():
    c2 = cases.c2_model()
    out = np.full((4, 6, 2), -7.0)
    noscale = Model.linear(Sde.ouProcess(1)).run(Parameters.apply(0.1, SdeParameter.ouParameter(0.0, 1.0, 0.2, 0.0, 0.3))).descriptor()
    noscale.leaf_array[0].has_scale = 0      # (the Python constructors refuse such a model themselves)
    t_df0 = Model.studentsT(Sde.ouProcess(1), 0).run(Parameters.apply(0.1, SdeParameter.ouParameter(0.0, 1.0, 0.2, 0.0, 0.3)))
    lgcp = Model.lgcp(Sde.ouProcess(1)).run(Parameters.apply(None, SdeParameter.ouParameter(0.0, 1.0, 0.2, 0.0, 0.3)))
    for args, word in (((c2, 2, 0.0, [1.0, 2.0, 3.0], None), "null argument"),
                       ((c2, 0, 0.0, [1.0, 2.0, 3.0], out), "n_paths"),
                       ((c2, 2, 0.0, [1.0, float("nan"), 3.0], out), "not finite"),
                       ((c2, 2, float("inf"), [1.0, 2.0, 3.0], out), "t0 is not finite"),
                       ((c2, 2, 2.0, [1.0, 2.0, 3.0], out), "is before t0"),
                       ((c2, 2, 0.0, [1.0, 3.0, 2.0], out), "non-decreasing"),
                       ((lgcp, 2, 0.0, [1.0, 2.0, 3.0], out), "log-Gaussian Cox"),
                       ((noscale, 2, 0.0, [1.0, 2.0, 3.0], out), "Must provide SD parameter"),
                       ((t_df0, 2, 0.0, [1.0, 2.0, 3.0], out), "df >= 1")):
        rc, msg = _raw(*args)
        assert rc == _abi.CSSM_EINVAL_ARG and word in msg, (word, rc, msg)
        assert np.all(out == -7.0), word
    lib = _abi.load_library()
    t = np.array([1.0])
    assert lib.cssm_simulate(None, 2, KEY, 0.0, t.ctypes.data_as(_dp), 1, 0, 0, out.ctypes.data_as(_dp)) == _abi.CSSM_EINVAL_ARG
    assert "null argument" in _abi.last_error()
    assert lib.cssm_simulate(c2.descriptor().ptr(), 2, KEY, 0.0, t.ctypes.data_as(_dp), 1, 0, 99, out.ctypes.data_as(_dp)) == _abi.CSSM_EINVAL_ARG
    assert "device 99 out of range" in _abi.last_error() and np.all(out == -7.0)
