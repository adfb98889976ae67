"""CPU-only: what the per-dimension and block-edge GPU tests of the fleet rest on.

1. The premises, on the oracle alone: the per-d fixture (cases.dim_model(d), S = 3, N = 257, six records with a gap) and the edge fleet
   (ragged_c2(6) at every EDGE_N) resample non-trivially and pass through the None branch, so a GPU test on them exercises resampling,
   the unweighted call sites and every row.
2. The block geometry: a Python mirror of fleet_create's block size (csrc/cssm_fleet.hip: `f->threads = ...`), of k_fleet_series' scan
   ranges it / j0 / j1 (csrc/cssm_fleet.hip.h) and of fleet_ranks' np2 (csrc/cssm_fleet.hip), and on it the facts that make EDGE_N edges
   -- and that no N the suite ran before them had a wholly idle wave.
3. The matrix: every FleetKind of csrc/cssm_fleet.hip.h and every k_fleet_* kernel dispatched over D in csrc/cssm_fleet*.hip is named
   here with the GPU test that runs it at d = 1 .. 16.  A new kind or a new dispatched kernel fails this file until it has one."""
import glob
import importlib
import os
import re

import numpy as np
import pytest

import cases
from oracle import oracle
from test_gpu_fleet import SEED, ragged_c2
from test_gpu_fleet_interpolate import with_gap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "composablestatespacemodels_amd", "csrc")

EDGE_N = [64, 65, 2049, 4095]                                  # tests/test_gpu_fleet_edges.py
OLD_N = [1, 2, 63, 100, 257, 1000, 4096]                       # every N list of the fleet tests before the edges ...
OLD_N_SINGLE = [64, 300, 500, 3000]                            # ... and the N single tests of those files run


def per_d_fixture(d):
    """(model, n, seeds, datas) of every test_every_latent_dimension of the fleet files that has a gap in its data"""
    S = 3
    return (cases.dim_model(d), 257, [SEED + 17 * k for k in range(S)],
            [with_gap(cases.poisson_counts(6, seed=SEED + k), 2, 4) for k in range(S)])


def walk(model, n, seed, data):
    """one series on the oracle: (minimum ESS over the weighted records, unweighted records, the fewest distinct ancestors a weighted
    record left, the final ancestors)"""
    t, y, has = data
    o = oracle.OraclePf(model.descriptor(), n, seed)
    o.init(float(np.min(t)))
    ess_w, unweighted, distinct = [], 0, n
    for s in range(len(t)):
        _, ess = o.step(float(t[s]), float(y[s]), bool(has[s]))      # (an OracleError fails the test: no series may fail)
        if has[s]:
            ess_w.append(ess)
            distinct = min(distinct, len(set(o.ancestors().tolist())))
        else:
            unweighted += 1
    return min(ess_w), unweighted, distinct, o.ancestors()


# 1 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", list(range(1, 17)))
def test_premise_the_per_dimension_fixture_resamples_and_has_a_gap(d):
    """seen over d = 1 .. 16: minimum ESS 42 .. 204 of 257, 102 .. 203 distinct ancestors behind the harshest resampling, two unweighted
    records each"""
    model, n, seeds, datas = per_d_fixture(d)
    seen = []
    for k in range(3):
        ess, unweighted, distinct, anc = walk(model, n, seeds[k], datas[k])
        seen.append((ess, unweighted, distinct))
        assert ess < n, (d, k, ess)
        assert distinct < n and not np.array_equal(anc, np.arange(n)), (d, k)
        assert unweighted >= 1, (d, k)
        assert bool(datas[k][2][-1]), "the last record is weighted: the final ancestors are a resampling's"
    print(f"d = {d}: (min ESS, unweighted records, fewest distinct ancestors) per series {seen}")


@pytest.mark.parametrize("n", EDGE_N)
def test_premise_the_edge_fleet_resamples_and_has_gaps(n):
    """ragged_c2(6): series 0 and 3 are drawn without missing observations (cases.poisson_counts(missing=0)), the other four with; every
    series is weighed below ESS = N at least once and resampled non-trivially, and the None branch is taken in four of the six blocks
    of every launch (a series whose LAST record is unweighted ends on the identity the None branch writes: both endings occur)."""
    models, seeds, datas = ragged_c2(6)
    seen = []
    for k in range(6):
        ess, unweighted, distinct, anc = walk(models[k], n, seeds[k], datas[k])
        seen.append((ess, unweighted, distinct))
        assert ess < n, (n, k, ess)
        assert distinct < n, (n, k)                            # some weighted record's resampling dropped particles ...
        # ... and the ancestors the series ends on are a resampling's unless its last record is unweighted (then: the identity)
        assert np.array_equal(anc, np.arange(n)) == (not datas[k][2][-1]), (n, k)
        assert (unweighted >= 1) == (k % 3 != 0), (n, k, unweighted)
    print(f"N = {n}: (min ESS, unweighted records, fewest distinct ancestors) per series {seen}")


# 2 ------------------------------------------------------------------------------------------------------------------------------
def threads_of(n):
    """fleet_create (csrc/cssm_fleet.hip): f->threads = min(CSSM_FLEET_MAX_THREADS, max(64, ((n + 3) / 4 + 63) & ~63))"""
    return min(512, max(64, ((n + 3) // 4 + 63) & ~63))


def scan_range(n, tid):
    """k_fleet_series (csrc/cssm_fleet.hip.h): it = (n + bs - 1) / bs; j0 = tid * it; j1 = min(j0 + it, n) -- j0 >= n: an empty range"""
    bs = threads_of(n)
    it = (n + bs - 1) // bs
    j0 = tid * it
    return it, j0, (j0 + it if j0 + it < n else n)


def np2_of(n):
    """fleet_ranks (csrc/cssm_fleet.hip): the power of two >= max(n, 2) a row's sort in LDS pads to"""
    p = 2
    while p < n:
        p <<= 1
    return p


def owners(n):
    """the threads of the block that own at least one particle in the scan phases"""
    return [tid for tid in range(threads_of(n)) if scan_range(n, tid)[1] < scan_range(n, tid)[2]]


def idle_waves(n):
    busy = {tid >> 6 for tid in owners(n)}
    return [w for w in range(threads_of(n) >> 6) if w not in busy]


def test_the_mirror_reads_the_formulas_the_sources_state():
    """the three statements the mirror copies are still in the sources, word for word"""
    host = open(os.path.join(CSRC, "cssm_fleet.hip")).read()
    dev = open(os.path.join(CSRC, "cssm_fleet.hip.h")).read()
    assert "std::min<uint32_t>(CSSM_FLEET_MAX_THREADS, std::max<uint32_t>(64u, ((n + 3u) / 4u + 63u) & ~63u))" in host
    assert "while (r.np2 < n) r.np2 <<= 1;" in host and "FleetRowRanks{" in host and ", 2u};" in host
    assert "const uint32_t it = (n + bs - 1u) / bs;" in dev and "const uint32_t j0 = tid * it;" in dev
    assert "const uint32_t j1 = (j0 + it < n) ? j0 + it : n;" in dev
    assert re.search(r"#define\s+CSSM_FLEET_MAX_THREADS\s+512\b", dev)


def test_geometry_of_the_edge_sizes():
    # 2049: 512 threads of 5 particles; threads 410 .. 511 own nothing, so wave 7 (448 .. 511) is idle as a whole; the most padding
    assert threads_of(2049) == 512 and scan_range(2049, 0)[0] == 5
    assert owners(2049) == list(range(410)) and idle_waves(2049) == [7]
    assert scan_range(2049, 409)[1:] == (2045, 2049)
    assert np2_of(2049) == 4096 and np2_of(2049) - 2049 == 2047
    assert all(np2_of(n) - n <= 2047 for n in range(1, 4097))
    # 4095: 512 threads of 8, the last one short by one; one pad key
    assert threads_of(4095) == 512 and scan_range(4095, 0)[0] == 8
    assert owners(4095) == list(range(512)) and scan_range(4095, 511)[1:] == (4088, 4095)
    assert np2_of(4095) - 4095 == 1
    # 64: one full wave, one particle per thread, nothing idle, nothing padded
    assert threads_of(64) == 64 and scan_range(64, 63) == (1, 63, 64) and owners(64) == list(range(64)) and np2_of(64) == 64
    # 65: one wave, two particles per thread; lanes 33 .. 63 idle inside the only wave, lane 32 owns the single last particle
    assert threads_of(65) == 64 and scan_range(65, 0)[0] == 2
    assert owners(65) == list(range(33)) and scan_range(65, 32)[1:] == (64, 65) and idle_waves(65) == []
    assert np2_of(65) == 128


def test_no_size_the_suite_ran_before_had_a_wholly_idle_wave():
    """the statement of the gap: at every N of the older lists each wave of the block owns particles, so the wave sums, the max-scan
    carry and the lane-63 hand-offs of k_fleet_series never met a wave with nothing to hand on"""
    for n in OLD_N + OLD_N_SINGLE:
        assert idle_waves(n) == [], (n, idle_waves(n))
    assert [n for n in EDGE_N if idle_waves(n)] == [2049]
    # (where it can happen at all: only with 512 threads, i.e. 2049 <= N, and an `it` that leaves 64 threads over)
    assert min(n for n in range(1, 4097) if idle_waves(n)) == 2049


# 3 ------------------------------------------------------------------------------------------------------------------------------
# which GPU test runs the instantiation at every latent dimension: (module, function)
KIND_TESTS = {
    "plain": ("test_gpu_fleet", "test_every_latent_dimension"),
    "path": ("test_gpu_fleet_filter", "test_every_latent_dimension"),
    "hist": ("test_gpu_fleet_interpolate", "test_every_latent_dimension"),
    "ival": ("test_gpu_fleet_intervals", "test_every_latent_dimension"),
    "fcst": ("test_gpu_fleet_filter_forecasts", "test_every_latent_dimension"),
    "ring": ("test_gpu_fleet_step_interpolate", "test_every_latent_dimension"),
}
KERNEL_TESTS = {
    "k_fleet_summary": ("test_gpu_fleet_intervals", "test_every_latent_dimension"),          # (the twin fleet's summary)
    "k_fleet_forecast": ("test_gpu_fleet_forecast", "test_every_latent_dimension"),
    "k_fleet_forecast_post": ("test_gpu_fleet_forecast_posterior", "test_every_latent_dimension"),
    "k_fleet_lineage": ("test_gpu_fleet_interpolate", "test_every_latent_dimension"),
    "k_fleet_window": ("test_gpu_fleet_step_interpolate", "test_every_latent_dimension"),
}
# what the test has to call for the instantiation to run at all (fcst, ring: the helpers that make the call and hold it)
CALLS = {"plain": ".ll_filter(", "path": ".filter(", "hist": ".interpolate(", "ival": ".filter_intervals(", "fcst": "assert_whole_fleet_equals_the_loop(",
         "ring": "stream_and_check(", "k_fleet_summary": ".summary(", "k_fleet_forecast": ".forecast(",
         "k_fleet_forecast_post": ".forecast_posterior(", "k_fleet_lineage": ".interpolate(", "k_fleet_window": "stream_and_check("}


def fleet_kinds():
    src = open(os.path.join(CSRC, "cssm_fleet.hip.h")).read()
    m = re.search(r"enum\s+class\s+FleetKind\s*:\s*int\s*\{([^}]*)\}", src)
    assert m, "enum class FleetKind is gone from cssm_fleet.hip.h"
    return [w.strip() for w in m.group(1).split(",") if w.strip()]


def dispatched_kernels():
    names = set()
    for path in sorted(glob.glob(os.path.join(CSRC, "cssm_fleet*.hip"))):
        names.update(re.findall(r"DISPATCH_D\([^;]*?\b(k_fleet_\w+)<D>", open(path).read(), flags=re.S))
    return sorted(names)


def d_list_of(module, function):
    """the values of the test's parametrize mark over `d` (None without one), and the test's source"""
    fn = getattr(importlib.import_module(module), function, None)
    assert fn is not None, f"{module}::{function} does not exist"
    import inspect
    for mark in getattr(fn, "pytestmark", []):
        if mark.name == "parametrize" and mark.args[0] == "d":
            return list(mark.args[1]), inspect.getsource(fn)
    return None, inspect.getsource(fn)


def test_every_kind_and_every_dispatched_kernel_has_a_test_over_all_sixteen_dimensions():
    kinds, kernels = fleet_kinds(), dispatched_kernels()
    assert set(kinds) == set(KIND_TESTS), f"a FleetKind without a per-dimension test (or a stale entry): {set(kinds) ^ set(KIND_TESTS)}"
    assert set(kernels) == set(KERNEL_TESTS), f"a dispatched kernel without a per-dimension test: {set(kernels) ^ set(KERNEL_TESTS)}"
    # the launcher of cssm_fleet_d.hip names every kind, so each of the sixteen objects holds all of them
    launcher = open(os.path.join(CSRC, "cssm_fleet_d.hip")).read()
    assert sorted(re.findall(r"case\s+FleetKind::(\w+)\s*:", launcher)) == sorted(kinds)
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "CSSM_FLEET_D" in mk
    for what, (module, function) in {**KIND_TESTS, **KERNEL_TESTS}.items():
        ds, source = d_list_of(module, function)
        assert ds == list(range(1, 17)), (what, module, function, ds)
        assert "cases.dim_model(d)" in source and CALLS[what] in source, (what, module, function)
        mod = importlib.import_module(module)
        marks = mod.pytestmark if isinstance(mod.pytestmark, list) else [mod.pytestmark]
        assert any(m.name == "gpu" for m in marks), module
