"""Forecasts from a joint posterior sample on a host without a GPU: the pair draw of include/cssm_obs_draws.h (cssm_posterior_pick,
built with gcc as tests/cpp/posterior_pick_twin.c), the entry point's declaration and binding, the burn-in / thinning of a chain's output
arrays against formats.read_pmmh_json, and the loud failure without a device."""
from __future__ import annotations

import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import cases
from composablestatespacemodels_amd import _abi, load_library
from composablestatespacemodels_amd import formats as F
from composablestatespacemodels_amd.filter import ParticleFilter
from composablestatespacemodels_amd.pmmh import MetropState, posterior_rows

stats = pytest.importorskip("scipy.stats")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEY = 0x0B5E_55ED
_u32p = C.POINTER(C.c_uint32)


def build_pick_twin(out_dir) -> C.CDLL:
    so = os.path.join(str(out_dir), "posterior_pick_twin.so")
    subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-mfma", "-std=c99", "-shared", "-fPIC", "-o", so,
                           os.path.join(ROOT, "tests", "cpp", "posterior_pick_twin.c"), "-lm"])
    lib = C.CDLL(so)
    lib.twin_posterior_picks.argtypes = [C.c_uint64, C.c_size_t, C.c_uint64, _u32p]
    lib.twin_posterior_picks.restype = None
    return lib


def twin_picks(lib, key, n, M) -> np.ndarray:
    out = np.zeros(n, dtype=np.uint32)
    lib.twin_posterior_picks(key, n, M, out.ctypes.data_as(_u32p))
    return out


@pytest.fixture(scope="module")
def pick_twin(tmp_path_factory):
    return build_pick_twin(tmp_path_factory.mktemp("pick_twin"))


def test_picks_are_deterministic_and_in_range(pick_twin):
    a = twin_picks(pick_twin, KEY, 50_000, 1000)
    b = twin_picks(pick_twin, KEY, 50_000, 1000)
    assert np.array_equal(a, b)
    assert a.max() < 1000
    # a particle's pick depends on (key, i) alone: a prefix of a longer draw, and another key draws otherwise
    assert np.array_equal(twin_picks(pick_twin, KEY, 100, 1000), a[:100])
    assert np.mean(twin_picks(pick_twin, KEY + 1, 50_000, 1000) == a) < 0.01
    assert not np.any(twin_picks(pick_twin, KEY, 1000, 1))


@pytest.mark.parametrize("M", [7, 1000])
def test_picks_are_uniform(pick_twin, M):
    n = 200_000
    counts = np.bincount(twin_picks(pick_twin, KEY, n, M), minlength=M)
    assert counts.size == M
    assert stats.chisquare(counts).pvalue > 1e-4


def test_posterior_symbol_is_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "cssm_pf.h")).read()
    assert re.search(r"int cssm_pf_forecast_posterior\(cssm_pf\* pf, const cssm_model_desc\* desc", header)
    assert "#define CSSM_STREAM_POST 9u" in open(os.path.join(ROOT, "include", "cssm_obs_draws.h")).read()
    lib = load_library()
    assert "cssm_pf_forecast_posterior" in {s[0] for s in _abi.SYMBOLS}
    assert hasattr(lib, "cssm_pf_forecast_posterior")
    x = np.zeros(3)
    rc = lib.cssm_pf_forecast_posterior(None, None, x.ctypes.data_as(C.POINTER(C.c_double)), 1, x.ctypes.data_as(C.POINTER(C.c_double)),
                                        1, 0.0, None, 0, None, KEY, 0.975, *([None] * 11))
    assert rc == _abi.CSSM_EINVAL_ARG and b"null handle" in lib.cssm_last_error()


@pytest.mark.parametrize("burn_in,thin", [(0, 1), (3, 1), (4, 3), (0, 5), (12, 4), (20, 1)])
def test_array_burn_in_and_thinning_select_what_the_json_reader_selects(tmp_path, burn_in, thin):
    params = cases.c2_params()
    rng = np.random.default_rng(5)
    iters, nt = 17, len(params.flattenParams())
    theta = np.asarray(params.flattenParams()) + 0.1 * rng.standard_normal((iters, nt))
    last = rng.standard_normal((iters, 3))
    path = tmp_path / "chain.json"
    with open(path, "w") as f:
        for i in range(iters):
            f.write(F.metrop_state_to_json(MetropState(-10.0 - i, params.withFlat(theta[i]), last[i], i), 24.0, [1, 2]) + "\n")
    back = list(F.read_pmmh_json(str(path), burn_in, thin))
    th, xs = posterior_rows(theta, last, burn_in, thin)
    assert len(back) == th.shape[0] == xs.shape[0]
    for s, row, x in zip(back, th, xs):
        assert np.array_equal(np.asarray(s.params.flattenParams()), row)
        assert np.array_equal(np.asarray(s.sde), x)
    with pytest.raises(ValueError):
        posterior_rows(theta, last, -1, 1)
    with pytest.raises(ValueError):
        posterior_rows(theta, last, 0, 0)


def test_forecast_posterior_needs_a_parameter_tree_for_arrays():
    with pytest.raises(ValueError):
        ParticleFilter.forecastPosterior((np.zeros((2, 10)), np.zeros((2, 3))), cases.c2_unparam(), 0.0, [1.0], 64)
    with pytest.raises(ValueError):
        ParticleFilter.forecastPosterior([], cases.c2_unparam(), 0.0, [1.0], 64)


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="this check is for hosts without a GPU")
def test_posterior_forecasts_fail_loudly_without_gpu():
    params = cases.c2_params()
    post = [MetropState(-1.0, params, np.zeros(3), 1)]
    with pytest.raises(_abi.CssmError) as ei:
        ParticleFilter.forecastPosterior(post, cases.c2_unparam(), 0.0, [1.0, 2.0], 64)
    assert ei.value.code == _abi.CSSM_EHIP
