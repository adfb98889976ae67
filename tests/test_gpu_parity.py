"""-m gpu: the HIP path (through the C ABI) against the oracle on the same seeded inputs.

Bar (BASELINE.json north star): ancestor index arrays bit-exact; marginal log-likelihood within a
stated fp64 tolerance.  Because CPU and GPU share the numerics contract (include/cssm_numerics.h)
the tolerance used here is ZERO: particles, log-weights, ancestors, ll and ess must be identical.
"""
import numpy as np
import pytest

import cases
from composablestatespacemodels_amd.filter import NativePf, Resampling
from oracle import oracle

pytestmark = pytest.mark.gpu


def _assert_weights_match(g, o_logw, o=None, err_msg=""):
    """The handle keeps either the log-weights of the last weighted step or -- the fused kernel -- the weights
    w1 = exp(min(w - c, 2^-20)) relative to the observation's reference level c in their place (what stepFilter hands its
    resampler, ParticleFilter.scala:125-126, rescaled by c instead of the max).  Whichever it keeps must equal what the oracle's
    log-weights give, bit for bit; with the whole-cloud oracle at hand the level must be the oracle's too."""
    w = g.weights()
    if w is None:
        np.testing.assert_array_equal(g.logw(), o_logw, err_msg="log-weights: " + err_msg)
        return
    w1, c = w
    if o is not None:
        assert c == o.ref()[0], (c, o.ref(), err_msg)
    lw = np.where(np.isnan(o_logw), -np.inf, o_logw)
    np.testing.assert_array_equal(w1, oracle.c_exp(np.minimum(lw - c, 2.0 ** -20)), err_msg="weights: " + err_msg)


def _compare_streaming(model, n, t, y, has, seed=cases.SEED, lgcp_precision=0, fused=0):
    g = NativePf(model, n, seed, lgcp_precision=lgcp_precision)
    g.set_option(3, fused)      # CSSM_OPT_FUSED_SUMS
    o = oracle.OraclePf(model.descriptor(lgcp_precision), n, seed)
    t0 = float(np.min(t))
    g.init(t0); o.init(t0)
    np.testing.assert_array_equal(g.particles(), o.particles())
    for s in range(len(t)):
        gl, ge = g.step(t[s], y[s], bool(has[s]))
        ol, oe = o.step(t[s], y[s], bool(has[s]))
        np.testing.assert_array_equal(g.proposed(), o.proposed(), err_msg=f"propagated cloud differs at step {s}")
        if has[s] or lgcp_precision:
            _assert_weights_match(g, o.logw(), o, err_msg=f"step {s}")
            np.testing.assert_array_equal(g.ancestors(), o.ancestors(), err_msg=f"ancestors differ at step {s}")
        np.testing.assert_array_equal(g.particles(), o.particles(), err_msg=f"resampled cloud differs at step {s}")
        assert gl == ol, f"ll differs at step {s}: {gl!r} vs {ol!r}"
        assert ge == oe, f"ess differs at step {s}"
    g.close()


@pytest.mark.parametrize("n", [1, 2, 63, 64, 1000, 1023, 1024, 1025, 4096, 5000])
def test_c1_streaming_bit_exact(n):
    t, y, has = cases.poisson_counts(12)
    _compare_streaming(cases.c1_model(), n, t, y, has)


@pytest.mark.parametrize("name", ["c2_model", "c3_model", "gen_brownian_seasonal_gaussian", "euler_model", "linear_model"])
def test_models_streaming_bit_exact(name):
    model = getattr(cases, name)()
    if name in ("gen_brownian_seasonal_gaussian", "linear_model"):
        t, y, has = cases.gaussian_series(10)
    else:
        t, y, has = cases.poisson_counts(10)
    _compare_streaming(model, 3000, t, y, has)


@pytest.mark.parametrize("name", ["negbin", "zip", "bernoulli", "studentt", "beta"])
def test_next_row_observation_models_streaming_bit_exact(name):
    """NegBin, ZIP, Bernoulli, Student-t, Beta through the same kernels and boundary."""
    model, t, y, has = cases.golden_case(name, 9)
    _compare_streaming(model, 2500, t, y, has)


def test_maximum_dimension_and_leaf_count():
    """d = 16 (CSSM_MAX_DIM) over three leaves, and 16 leaves (CSSM_MAX_LEAVES)."""
    t, y, has = cases.poisson_counts(6)
    _compare_streaming(cases.max_dim_model(), 1500, t, y, has)
    _compare_streaming(cases.many_leaves_model(), 1200, t, y, has)


def test_independent_handles_driven_concurrently_and_one_handle_from_several_threads():
    """SURVEY.md 8b, threading: Akka calls stepFilter one at a time but from different dispatcher threads, and independent
    handles run side by side (two PMMH chains under mapAsync(2), examples/DetermineParameters.scala:68-69).  Three
    handles with different models and sizes are driven from three threads at once (ctypes releases the GIL: the calls
    really overlap), each alternating batch and streaming calls; then one handle is stepped from a fresh thread per
    observation.  Everything must equal what the same calls give one after the other."""
    import threading
    jobs = [(cases.c2_model(), 40000, cases.poisson_counts(30), 11), (cases.c3_model(), 20000, cases.poisson_counts(25), 12),
            (cases.c1_model(), 100000, cases.poisson_counts(35), 13)]

    def work(model, n, data, seed, out):
        t, y, has = data
        pf = NativePf(model, n, seed)
        res = []
        for rep in range(3):
            res.append(pf.run(t, y, has)[0])
            pf.init(float(t[0]))
            for s in range(len(t)):
                ll, ess = pf.step(t[s], y[s], bool(has[s]))
            res.append((ll, ess))
        res.append(pf.particles().copy())
        pf.close()
        out.append(res)

    serial = []
    for j in jobs:
        o = []; work(*j, o); serial.append(o[0])
    outs = [[] for _ in jobs]
    threads = [threading.Thread(target=work, args=(*j, o)) for j, o in zip(jobs, outs)]
    for th in threads: th.start()
    for th in threads: th.join()
    for o, ref in zip(outs, serial):
        assert len(o) == 1, "a worker thread raised"
        assert o[0][:-1] == ref[:-1]
        np.testing.assert_array_equal(o[0][-1], ref[-1])
    # one handle, a different thread for every call
    model, n, (t, y, has), seed = jobs[0]
    a = NativePf(model, n, seed); a.init(float(t[0]))
    got = []
    for s in range(len(t)):
        th = threading.Thread(target=lambda s=s: got.append(a.step(t[s], y[s], bool(has[s]))))
        th.start(); th.join()
    assert got[-1] == serial[0][1]
    a.close()


def test_single_datum_all_missing_and_empty_series():
    from composablestatespacemodels_amd import CssmError
    model = cases.c2_model()
    g = NativePf(model, 700, cases.SEED)
    o = oracle.OraclePf(model.descriptor(), 700, cases.SEED)
    # T = 1: the first datum has dt = 0 (t0 = min t), ParticleFilter.scala:138
    assert g.run(np.array([3.0]), np.array([2.0]))[0] == o.filter(np.array([3.0]), np.array([2.0]))[0]
    # every observation missing: particles are only propagated, ll stays 0 and ess stays N (:121)
    t = np.arange(5.0); y = np.zeros(5); has = np.zeros(5, dtype=np.uint8)
    ll, ll_t, ess_t, _ = g.run(t, y, has)
    oll, oll_t, oess_t, _ = o.filter(t, y, has)
    assert ll == 0.0 == oll and list(ess_t) == [700] * 5 == list(oess_t)
    np.testing.assert_array_equal(g.particles(), o.particles())
    np.testing.assert_array_equal(g.ancestors(), np.arange(700))
    # empty data: the reference's minBy throws on an empty Vector
    with pytest.raises(CssmError) as e:
        g.run(np.array([]), np.array([]))
    assert e.value.code == -6
    g.close()


def test_decreasing_time_is_reported_as_nonfinite():
    """A negative dt makes sqrt(sigma*dt) NaN in the reference too (Sde.scala:117); here it is an error code."""
    from composablestatespacemodels_amd import CssmError
    g = NativePf(cases.c1_model(), 256, 1)
    g.init(5.0)
    with pytest.raises(CssmError) as e:
        g.step(4.0, 1.0)
    assert e.value.code == -5
    g.close()


def test_missing_observations_bit_exact():
    t, y, has = cases.poisson_counts(16, missing=0.4)
    assert has.sum() < 16
    _compare_streaming(cases.c2_model(), 2048, t, y, has)


def test_irregular_times_and_unsorted_t0():
    t = np.array([0.0, 0.5, 0.5, 2.25, 3.0, 7.5])
    y = np.array([1.0, 0.0, 3.0, 2.0, 2.0, 5.0])
    _compare_streaming(cases.c2_model(), 1500, t, y, np.ones(6, dtype=np.uint8))


def test_lgcp_streaming_bit_exact():
    t, y, has = cases.event_times(8)
    _compare_streaming(cases.c4_model(), 2000, t, y, has, lgcp_precision=2)


@pytest.mark.parametrize("name,n,T", [("c1_model", 1000, 100), ("c2_model", 8192, 40), ("c3_model", 4096, 30)])
def test_batch_ll_filter_matches_oracle(name, n, T):
    model = getattr(cases, name)()
    t, y, has = cases.poisson_counts(T, missing=0.1)
    g = NativePf(model, n, cases.SEED)
    with pytest.raises(Exception):          # (no batch call yet, and the event pair is opt-in: CSSM_OPT_LOOP_EVENTS)
        g.last_loop_ms()
    g.set_option(9, 1)
    o = oracle.OraclePf(model.descriptor(), n, cases.SEED)
    gl, gll, gess, gpath = g.run(t, y, has, want_path=True)
    ol, oll, oess, opath = o.filter(t, y, has, want_path=True)
    assert gl == ol
    np.testing.assert_array_equal(gll, oll)
    np.testing.assert_array_equal(gess, oess)
    np.testing.assert_array_equal(gpath, opath)
    np.testing.assert_array_equal(g.ancestors(), o.ancestors())
    np.testing.assert_array_equal(g.particles(), o.particles())
    assert g.last_loop_ms() > 0.0
    # llFilter (no path) gives the same likelihood
    assert g.run(t, y, has)[0] == ol
    g.close()


@pytest.mark.parametrize("name", cases.GOLDEN_NAMES)
def test_gpu_reproduces_committed_golden_runs(name):
    """tests/golden/oracle_runs.json was produced in the build container (tests/golden/make_golden.py)."""
    import json, os
    g = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "oracle_runs.json")))[name]
    model, t, y, has = cases.golden_case(name, g["T"], g["missing"])
    pf = NativePf(model, g["n"], cases.SEED, lgcp_precision=g["lgcp_precision"])
    ll, ll_t, ess_t, path = pf.run(t, y, has, want_path=True)
    assert ll == float.fromhex(g["ll"])
    np.testing.assert_array_equal(ll_t, [float.fromhex(v) for v in g["ll_t"]])
    np.testing.assert_array_equal(ess_t, g["ess_t"])
    np.testing.assert_array_equal(pf.ancestors(), g["ancestors_last"])
    np.testing.assert_array_equal(path, [[float.fromhex(v) for v in row] for row in g["path"]])
    pf.close()


def test_filter_interface_mirrors_the_reference():
    """Filter(mod, resample).llFilter / filter / filterStream (ParticleFilter.scala:137-166)."""
    from composablestatespacemodels_amd import Data
    from composablestatespacemodels_amd.filter import Filter, ParticleFilter
    model = cases.c2_model()
    t, y, has = cases.poisson_counts(9, missing=0.2)
    data = [Data(float(a), float(b) if h else None) for a, b, h in zip(t, y, has)]
    o = oracle.OraclePf(model.descriptor(), 1000, cases.SEED)
    oll, oll_t, oess, opath = o.filter(t, y, has, want_path=True)
    f = Filter(model, Resampling.systematicResampling)
    assert f.llFilter(data, 1000) == oll
    ll, states = f.filter(data, 1000)
    assert ll == oll and len(states) == len(data) + 1 and states[0].time == 0.0
    np.testing.assert_array_equal(np.array([s.state for s in states]), opath)
    assert ParticleFilter.likelihood(data, Resampling.systematicResampling, 1000)(model) == oll
    # filterStream: Flow.scan emits the initial state, then one PfState per datum
    out = list(f.filterStream(0.0, 1000)(iter(data)))
    assert len(out) == len(data) + 1 and out[0].ll == 0.0 and out[0].ess == 1000 and out[0].observation is None
    np.testing.assert_array_equal([s.ll for s in out[1:]], oll_t)
    np.testing.assert_array_equal([s.ess for s in out[1:]], oess)
    np.testing.assert_array_equal(out[-1].particles, o.particles())
    with pytest.raises(RuntimeError):
        out[0].particles    # an old PfState's cloud no longer exists on the device


def test_filter_init_replicates_the_given_state():
    from composablestatespacemodels_amd.filter import FilterInit
    model = cases.c2_model()
    f = FilterInit(model, Resampling.systematicResampling, [0.1, -0.2, 0.3])
    s = f.initialiseState(500, 2.0)
    np.testing.assert_array_equal(s.particles, np.tile(np.array([[0.1], [-0.2], [0.3]]), (1, 500)))
    o = oracle.OraclePf(model.descriptor(), 500, 20260101)
    o.init_from(2.0, [0.1, -0.2, 0.3])
    s2 = f.stepFilter(s, __import__("composablestatespacemodels_amd").Data(3.0, 2.0))
    oll, oess = o.step(3.0, 2.0)
    assert (s2.ll, s2.ess) == (oll, oess)
    np.testing.assert_array_equal(s2.particles, o.particles())


def test_lgcp_batch_matches_oracle():
    model = cases.c4_model()
    t, y, has = cases.event_times(12)
    g = NativePf(model, 4096, cases.SEED, lgcp_precision=2)
    o = oracle.OraclePf(model.descriptor(2), 4096, cases.SEED)
    gl, gll, gess, _ = g.run(t, y, has)
    ol, oll, oess, _ = o.filter(t, y, has)
    assert gl == ol
    np.testing.assert_array_equal(gess, oess)
    g.close()


@pytest.mark.parametrize("precision", [1, 2])
def test_lgcp_with_time_dependent_f_matches_oracle(precision):
    """Model.lgcp(...) |+| Model.seasonal(...): FilterLgcp.calcWeight evaluates f(x_k, tau_k) at every simulated time tau_k =
    t + k delta, the clock starting at the observation's time (model/ParticleFilter.scala:193-205,:215; model/Sde.scala:57-66).
    The kernel reads the seasonal coefficients of every sub-step from a per-observation table; streaming and batch, bit for
    bit against the oracle (oracle/cssm_oracle.c, step_lgcp)."""
    model = cases.lgcp_seasonal_model()
    t, y, has = cases.event_times(9, horizon=30.0)
    _compare_streaming(model, 3000, t, y, has, lgcp_precision=precision)
    g = NativePf(model, 5000, cases.SEED, lgcp_precision=precision)
    o = oracle.OraclePf(model.descriptor(precision), 5000, cases.SEED)
    gl, gll, gess, _ = g.run(t, y, has)
    ol, oll, oess, _ = o.filter(t, y, has)
    assert gl == ol
    np.testing.assert_array_equal(gll, oll)
    np.testing.assert_array_equal(gess, oess)
    np.testing.assert_array_equal(g.particles(), o.particles())
    # the cycle matters: the same series through a model without the seasonal leaf's time dependence differs
    flat = NativePf(cases.c4_model(), 5000, cases.SEED, lgcp_precision=precision)
    assert flat.run(t, y, has)[0] != gl
    flat.close()
    g.close()


@pytest.mark.parametrize("n", [1, 7, 1024, 1500, 100_000])
def test_stateless_resampler_matches_oracle(n):
    rng = np.random.default_rng(n)
    for kind in range(5):
        if kind == 0:
            w = rng.random(n)
        elif kind == 1:
            w = np.exp(-rng.exponential(20.0, n)); w[rng.integers(n)] = 1.0
        elif kind == 2:
            w = np.ones(n)
        elif kind == 3:
            w = np.zeros(n); w[rng.integers(n)] = 1.0
        else:
            w = rng.random(n); w[rng.random(n) < 0.7] = 0.0; w[rng.integers(n)] = 0.5
        for u in (0.0, float(rng.random()), 1.0 - 2.0**-53):
            np.testing.assert_array_equal(Resampling.systematicAncestors(w, u), oracle.resample_systematic(w, u))


@pytest.mark.parametrize("n", [1, 7, 1000, 1024, 4097, 200000])
def test_stateless_stratified_and_multinomial_match_oracle(n):
    """The `Resample[A]` seam for the other two resamplers (Resampling.scala:78-96): same ancestors as the oracle for the
    same (seed, step), and as the filter's own resampling step selects (tested through the filters elsewhere)."""
    rng = np.random.default_rng(n + 1)
    for case in range(3):
        w = rng.random(n) if case == 0 else np.exp(-rng.exponential(8.0, n))
        if case == 2:
            w[rng.random(n) < 0.5] = 0.0; w[rng.integers(n)] = 0.25
        for seed, step in ((cases.SEED, 0), (12345, 17)):
            np.testing.assert_array_equal(Resampling.ancestors(1, w, seed=seed, step=step), oracle.resample_stratified(w, seed, step))
            if n <= 20000:   # (the oracle scans linearly per draw, as Multinomial.draw does)
                np.testing.assert_array_equal(Resampling.ancestors(2, w, seed=seed, step=step), oracle.resample_multinomial(w, seed, step))
    out = Resampling.stratifiedResampling(list(range(n)), list(w), seed=3)
    assert len(out) == n and all(w[i] > 0 for i in out)
    out = Resampling.multinomialResampling(list(range(n)), list(w))
    assert len(out) == n and all(w[i] > 0 for i in out)


@pytest.mark.parametrize("n", [1, 4, 7, 1000, 1024, 4097, 200000, (1 << 20) + 3])
def test_residual_resampling_extension_matches_oracle(n):
    """cssm_resample_residual -- an EXTENSION: the resampler Resampling.scala:124-129 DESCRIBES (its body, :130-146, cannot run) --
    against its oracle twin bit for bit, and against its definition: particle i holds floor(n w_i / sum w) slots in particle order,
    then m multinomial draws from the residual weights; every slot is taken by a particle of positive weight, the output has n slots
    (the reference's own property of a resampler, SamplingTest.scala:16-18)."""
    rng = np.random.default_rng(n + 11)
    for case in range(5):
        if case == 0:
            w = rng.random(n)
        elif case == 1:
            w = np.exp(-rng.exponential(8.0, n))
        elif case == 2:
            w = np.ones(n)
        elif case == 3:
            w = np.zeros(n); w[rng.integers(n)] = 1.0
        else:
            w = rng.random(n) * 2.0 ** -60; w[rng.random(n) < 0.6] = 0.0; w[rng.integers(n)] = 2.0 ** -61
        for seed, step in ((cases.SEED, 0), (987, 5)):
            anc = Resampling.residualAncestors(w, seed=seed, step=step)
            np.testing.assert_array_equal(anc, oracle.resample_residual(w, seed, step), err_msg=f"case {case}")
            assert len(anc) == n and np.all(w[anc] > 0)
            cnt = np.bincount(anc, minlength=n)
            k = np.floor(n * (w / w.sum()) * (1.0 - 1e-12)).astype(np.int64)      # (floor up to the last ulp of the quotient)
            assert np.all(cnt >= np.minimum(k, cnt + (k - cnt) * (np.abs(n * w / w.sum() - np.round(n * w / w.sum())) < 1e-9)))
            K = int(np.floor(n * (w / w.sum())).sum())
            head = anc[:max(K - 2, 0)]
            assert np.all(np.diff(head.astype(np.int64)) >= 0)                    # the copies come first, in particle order
    out = Resampling.residualResampling(list(range(n)), list(w))
    assert len(out) == n and all(w[i] > 0 for i in out)


def test_resample_seam_returns_same_length():
    # the reference's own property: SamplingTest.scala:16-18
    w = np.random.default_rng(5).random(777)
    out = Resampling.systematicResampling(list(range(777)), list(w))
    assert len(out) == 777


def test_full_size_c2_agrees_with_oracle_and_properties():
    """BASELINE config 2 size (N = 2^20), shortened T: oracle comparison still finishes in seconds."""
    model = cases.c2_model()
    n, T = 1 << 20, 6
    t, y, has = cases.poisson_counts(T)
    g = NativePf(model, n, cases.SEED)
    o = oracle.OraclePf(model.descriptor(), n, cases.SEED)
    gl, gll, gess, _ = g.run(t, y, has)
    ol, oll, oess, _ = o.filter(t, y, has)
    assert gl == ol
    np.testing.assert_array_equal(gess, oess)
    anc = g.ancestors()
    np.testing.assert_array_equal(anc, o.ancestors())
    assert np.all(np.diff(anc.astype(np.int64)) >= 0), "ancestors must be non-decreasing in the slot index"
    assert 1 <= gess.min() and gess.max() <= n
    g.close()


@pytest.mark.parametrize("name,n,T,lgcp", [("c3_model", 1 << 22, 5, 0), ("c4_model", 1 << 24, 4, 2)])
def test_full_size_c3_c4_size_independent_properties(name, n, T, lgcp):
    """BASELINE configs 3 (d = 9, N = 2^22) and 4 (LGCP, N = 2^24) at their full particle counts, where the one-thread
    oracle no longer finishes in seconds: properties that hold at any size.  Batch == streaming bit for bit, a second
    run reproduces the first, ancestors are non-decreasing, and every particle's offspring count is floor or ceil of
    N w_i / sum(w) (systematic resampling, Resampling.scala:63-72)."""
    model = getattr(cases, name)()
    t, y, has = (cases.event_times(T) if lgcp else cases.poisson_counts(T))
    a = NativePf(model, n, cases.SEED, lgcp_precision=lgcp)
    ll_a, llt_a, ess_a, _ = a.run(t, y, has)
    b = NativePf(model, n, cases.SEED, lgcp_precision=lgcp)
    b.init(float(np.min(t)))
    for s in range(T):
        ll_b, ess_b = b.step(t[s], y[s], bool(has[s]))
        assert ess_b == ess_a[s]
    assert ll_b == ll_a and np.isfinite(ll_a)
    assert 1 <= ess_a.min() and ess_a.max() <= n
    anc = a.ancestors()
    np.testing.assert_array_equal(anc, b.ancestors())
    assert np.all(np.diff(anc.astype(np.int64)) >= 0)
    kept = a.weights()                              # (weights relative to the reference level, or log-weights: LGCP)
    if kept is None:
        lw = a.logw().astype(np.longdouble)
        w = np.exp(lw - lw.max())
    else:
        w = kept[0].astype(np.longdouble)
    expect = (w * (np.longdouble(n) / w.sum())).astype(np.float64)
    counts = np.bincount(anc, minlength=n).astype(np.float64)
    assert counts.sum() == n
    assert np.max(np.abs(counts - expect)) < 1.0 + 1e-6
    # the same series on the same handle again: identical (re-initialised state, same seed)
    ll_c, _, ess_c, _ = a.run(t, y, has)
    assert ll_c == ll_a
    np.testing.assert_array_equal(ess_c, ess_a)
    a.close(); b.close()


def test_offspring_fast_path_equals_forced_exact_path():
    """k_offspring decides most end slots from an fp64 position estimate; forcing the exact contract
    predicate everywhere must give the same ancestors (and both equal the oracle)."""
    model = cases.c2_model()
    t, y, has = cases.poisson_counts(10)
    # 2^20: one tile per block, all 1025 blocks resident, the publisher first; 3 * 2^20 + 777: several tiles per block, a ragged
    # last tile (the rolled exact loop takes over every particle when forced, single particles otherwise)
    for n in (5000, 1 << 18, 1 << 20, (3 << 20) + 777):
        a = NativePf(model, n, cases.SEED)
        ra = a.run(t, y, has)
        for mode in (1, 2):     # every particle / every third particle (mixed masks per thread) through the exact predicate
            b = NativePf(model, n, cases.SEED)
            b.set_option(1, mode)
            rb = b.run(t, y, has)
            assert ra[0] == rb[0]
            np.testing.assert_array_equal(ra[2], rb[2])
            np.testing.assert_array_equal(a.ancestors(), b.ancestors())
            np.testing.assert_array_equal(a.particles(), b.particles())
            b.close()
        a.close()


@pytest.mark.parametrize("name,n", [("c2_model", 20000), ("c3_model", 5000), ("bernoulli_model", 3000), ("linear_model", 1 << 18)])
def test_device_summaries_match_oracle(name, n):
    """cssm_pf_summary == getIntervals (ParticleFilter.scala:415-424): order statistics exact, means to 1e-12."""
    model = getattr(cases, name)()
    t, y, has = {"bernoulli_model": cases.binary_series, "linear_model": cases.gaussian_series}.get(name, cases.poisson_counts)(6)
    g = NativePf(model, n, cases.SEED)
    o = oracle.OraclePf(model.descriptor(), n, cases.SEED)
    g.init(0.0); o.init(0.0)
    for s in range(6):
        g.step(t[s], y[s], bool(has[s])); o.step(t[s], y[s], bool(has[s]))
        gm, glo, ghi, gem, gel, geu = g.summary(0.975)
        om, olo, ohi, oem, oel, oeu = o.summary(0.975)
        np.testing.assert_array_equal(glo, olo)
        np.testing.assert_array_equal(ghi, ohi)
        assert (gel, geu) == (oel, oeu)
        np.testing.assert_allclose(gm, om, rtol=1e-12, atol=1e-13)
        assert abs(gem - oem) <= 1e-12 * max(1.0, abs(oem))
    g.close()


def test_get_intervals_mirror():
    from composablestatespacemodels_amd import Data
    from composablestatespacemodels_amd.filter import Filter, ParticleFilter
    model = cases.c2_model()
    f = Filter(model, Resampling.systematicResampling)
    s = f.initialiseState(4000, 0.0)
    s = f.stepFilter(s, Data(1.0, 3.0))
    out = ParticleFilter.getIntervals(model, s)
    assert out.time == 1.0 and out.observation == 3.0 and len(out.stateIntervals) == 3
    assert all(ci.lower < m < ci.upper for ci, m in zip(out.stateIntervals, out.state))
    assert out.etaIntervals.lower < out.eta < out.etaIntervals.upper
    # the named helpers of the reference (ParticleFilter.scala:455-512) against a host evaluation of the downloaded cloud
    x = s.particles
    np.testing.assert_allclose(ParticleFilter.meanState(s), x.mean(axis=1), rtol=1e-12)
    for interval in (0.975, 0.9):
        cis = ParticleFilter.getallCredibleIntervals(s, interval)
        n = x.shape[1]; index = int(np.floor(interval * n))
        for k, ci in enumerate(cis):
            srt = np.sort(x[k])
            assert (ci.lower, ci.upper) == (srt[n - index - 1], srt[index - 1])
    ci = ParticleFilter.getOrderStatistic(list(x[0]), 0.975)
    srt = np.sort(x[0]); index = int(np.floor(0.975 * len(srt)))
    assert (ci.lower, ci.upper) == (srt[len(srt) - index], srt[index])


@pytest.mark.parametrize("kind,flag", [(1, oracle.RESAMPLE_STRATIFIED), (2, oracle.RESAMPLE_MULTINOMIAL)])
@pytest.mark.parametrize("n", [1000, 5000, 1 << 16])
def test_stratified_and_multinomial_filters_bit_exact(kind, flag, n):
    """Filter(mod, Resampling.stratifiedResampling / multinomialResampling), Resampling.scala:78-96."""
    model = cases.c2_model()
    t, y, has = cases.poisson_counts(7, missing=0.2)
    g = NativePf(model, n, cases.SEED)
    g.set_option(2, kind)
    o = oracle.OraclePf(model.descriptor(), n, cases.SEED, flag)
    g.init(0.0); o.init(0.0)
    for s in range(len(t)):
        gl, ge = g.step(t[s], y[s], bool(has[s]))
        ol, oe = o.step(t[s], y[s], bool(has[s]))
        np.testing.assert_array_equal(g.ancestors(), o.ancestors(), err_msg=f"step {s}")
        np.testing.assert_array_equal(g.particles(), o.particles())
        assert (gl, ge) == (ol, oe)
    # batch driver too
    assert g.run(t, y, has)[0] == o.filter(t, y, has)[0]
    g.close()


def test_filter_accepts_the_three_resamplers():
    from composablestatespacemodels_amd import Data
    from composablestatespacemodels_amd.filter import Filter
    data = [Data(float(i), float(i % 3)) for i in range(5)]
    lls = [Filter(cases.c2_model(), r).llFilter(data, 4096) for r in
           (Resampling.systematicResampling, Resampling.stratifiedResampling, Resampling.multinomialResampling)]
    assert len(set(lls)) == 3 and max(lls) - min(lls) < 1.0


def test_cpp_host_mirror_matches_python_binding_and_oracle(tmp_path):
    """include/cssm_pf.hpp (C++ mirror of Filter/llFilter/filter/stepFilter) compiled with g++ and run here."""
    import os, subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "test_hpp")
    lib = os.path.join(root, "composablestatespacemodels_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I" + os.path.join(root, "include"), os.path.join(root, "tests", "cpp", "test_hpp.cpp"),
                           "-L" + lib, "-lcssm_pf", "-Wl,-rpath," + lib, "-o", exe])
    out = subprocess.run([exe, "4096"], capture_output=True, text=True, check=True).stdout
    kv = dict(line.split(" ", 1) for line in out.strip().splitlines())
    model = cases.c2_model()
    t = np.arange(8.0); y = np.array([2, 1, 4, 0, 3, 2, 5, 1.0]); has = np.ones(8, dtype=np.uint8); has[3] = 0
    o = oracle.OraclePf(model.descriptor(), 4096, cases.SEED)
    oll, _, oess, _ = o.filter(t, y, has)
    assert float.fromhex(kv["ll"]) == oll and float.fromhex(kv["ll_filter"]) == oll and float.fromhex(kv["ll_stream"]) == oll
    assert int(kv["path_len"]) == 9 and int(kv["ess"]) == oess[-1] and int(kv["error_code"]) == -1
    # cssm::Resampling (the Resample[A] seam) against the oracle's ancestors for the same weights
    w = np.array([(i * 37 % 101) / 101.0 + (5.0 if i == 500 else 0.0) for i in range(1000)])
    def h(anc):
        v = 0
        for a in anc:
            v = (v * 1000003 + int(a)) % (1 << 64)
        return v
    assert int(kv["resample_len"]) == 1000
    assert int(kv["resample_sys"]) == h(oracle.resample_systematic(w, 0.25))
    assert int(kv["resample_strat"]) == h(oracle.resample_stratified(w, 20260101, 3))
    assert int(kv["resample_multi"]) == h(oracle.resample_multinomial(w, 20260101, 3))


def test_errors_are_reported_not_swallowed():
    from composablestatespacemodels_amd import CssmError
    model = cases.linear_model()
    g = NativePf(model, 128, 1)
    with pytest.raises(CssmError):
        g.step(1.0, 1.0)  # step before init
    g.init(0.0)
    with pytest.raises(CssmError) as e:
        g.step(1.0, float("nan"))  # NaN log-weights: breeze's Gaussian/Poisson would throw
    assert e.value.code == -5
    g.close()


def _outlier_series(T=10, where=(4,)):
    t, y, has = cases.poisson_counts(T)
    y = y.copy()
    for s in where:
        y[s] = 60.0            # log p(60 | lambda ~ 2) is ~70 below the Poisson supremum: the reference level is ruled out
    return t, y, has


@pytest.mark.parametrize("fused", [0, 1])
@pytest.mark.parametrize("n", [1000, 1 << 16])
def test_outlying_observation_falls_back_to_the_max_streaming(n, fused):
    """cssm_ref_choose: a step whose max log-weight is > 32 below the observation's reference level is rescaled by
    the max (second attempt on the device), exactly as the oracle decides."""
    model = cases.c2_model()
    t, y, has = _outlier_series()
    o = oracle.OraclePf(model.descriptor(), n, cases.SEED)
    o.init(0.0)
    levels = []
    for s in range(len(t)):
        o.step(t[s], y[s], True)
        levels.append(o.ref())
    assert levels[4][0] == levels[4][1] and levels[3][0] != levels[3][1]   # max used at the outlier only
    _compare_streaming(model, n, t, y, has, fused=fused)


@pytest.mark.parametrize("fused", [0, 1])
@pytest.mark.parametrize("name,where", [("c2_model", (4,)), ("c2_model", (0, 9)), ("c3_model", (7,))])
def test_outlying_observation_batch_rerun_matches_oracle(name, where, fused):
    model = getattr(cases, name)()
    n = 5000
    t, y, has = _outlier_series(10, where)
    g = NativePf(model, n, cases.SEED)
    g.set_option(3, fused)
    gl, gll, gess, gpath = g.run(t, y, has, want_path=True)
    o = oracle.OraclePf(model.descriptor(), n, cases.SEED)
    ol, oll, oess, opath = o.filter(t, y, has, want_path=True)
    assert gl == ol
    np.testing.assert_array_equal(gll, oll)
    np.testing.assert_array_equal(gess, oess)
    np.testing.assert_array_equal(gpath, opath)
    np.testing.assert_array_equal(g.particles(), o.particles())
    # the handle is back in its ordinary mode afterwards
    t2, y2, has2 = cases.poisson_counts(10)
    assert g.run(t2, y2, has2)[0] == oracle.OraclePf(model.descriptor(), n, cases.SEED).filter(t2, y2, has2)[0]
    g.close()


@pytest.mark.parametrize("fused", [0, 1])
@pytest.mark.parametrize("n", [1000, 5000])
def test_outlying_observations_inside_a_continued_call(n, fused):
    """A held observation inside a CONTINUED call (run on records 0..3, run_more on 4..9): outliers at the continued call's first record
    and at its last; record 5 carries no datum, so the max-slot set and the validity of the ancestors at a held record are not functions
    of its index.  The state each redo starts from is derived from the call's starting state: against the oracle's filter of the whole
    series, bit for bit."""
    model = cases.c2_model()
    t, y, has = _outlier_series(10, (4, 9))
    has = has.copy(); has[5] = 0
    g = NativePf(model, n, cases.SEED)
    g.set_option(3, fused)
    _, ll_a, ess_a, _ = g.run(t[:4], y[:4], has[:4])
    gl, ll_b, ess_b = g.run_more(t[4:], y[4:], has[4:])
    o = oracle.OraclePf(model.descriptor(), n, cases.SEED)
    ol, oll, oess, _ = o.filter(t, y, has)
    assert gl == ol
    np.testing.assert_array_equal(np.concatenate([ll_a, ll_b]), oll)
    np.testing.assert_array_equal(np.concatenate([ess_a, ess_b]), oess)
    np.testing.assert_array_equal(g.particles(), o.particles())
    g.close()


def test_outlying_gaussian_observation_and_pmmh_path():
    model = cases.linear_model()
    n = 4096
    t, y, has = cases.gaussian_series(8)
    y = y.copy(); y[3] = 40.0           # ~80 sd away from every particle
    o = oracle.OraclePf(model.descriptor(), n, cases.SEED)
    want = o.filter(t, y, has)[0]
    for fused in (0, 1):
        g = NativePf(model, n, cases.SEED)
        g.set_option(3, fused)
        assert g.run(t, y, has)[0] == want
        g.close()


@pytest.mark.parametrize("name", ["c1_model", "c2_model", "c3_model", "linear_model", "negbin_model", "max_dim_model"])
@pytest.mark.parametrize("n", [2500, 1 << 17])
def test_fused_sums_equal_separate_pass(name, n):
    """CSSM_OPT_FUSED_SUMS: k_propagate forming the sums relative to the reference level (2 kernels per observation)
    gives the bits of the separate pass (3 kernels), streaming and batch, and both equal the oracle."""
    model = getattr(cases, name)()
    t, y, has = (cases.gaussian_series(7) if name == "linear_model" else cases.poisson_counts(7, missing=0.15))
    if n <= 4096:
        _compare_streaming(model, n, t, y, has, fused=1)
    runs = []
    for fused in (0, 1):
        g = NativePf(model, n, cases.SEED)
        g.set_option(3, fused)
        ll, ll_t, ess_t, _ = g.run(t, y, has)
        runs.append((ll, ll_t.copy(), ess_t.copy(), g.ancestors(), g.particles()))
        g.close()
    assert runs[0][0] == runs[1][0]
    for a, b in zip(runs[0][1:], runs[1][1:]):
        np.testing.assert_array_equal(a, b)
    assert runs[0][0] == oracle.OraclePf(model.descriptor(), n, cases.SEED).filter(t, y, has)[0]


def _contract_eval(fn, x, n_out):
    import ctypes as C
    from composablestatespacemodels_amd import _abi
    lib = _abi.load_library()
    x = np.ascontiguousarray(x, dtype=np.float64); out = np.zeros(n_out)
    dp = C.POINTER(C.c_double)
    _abi.check(lib.cssm_contract_eval(0, fn, x.ctypes.data_as(dp), x.size, out.ctypes.data_as(dp), out.size))
    return out


def test_contract_functions_on_the_device_match_the_host():
    """include/cssm_numerics.h compiled by hipcc for gfx950 (one-instruction min/max/ldexp forms) and by gcc for the
    host (portable forms) must agree bit for bit, function by function, on dense samples and on the edge cases."""
    rng = np.random.default_rng(2026)
    edge = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 710.0, 709.782712893384, np.nextafter(709.782712893384, 1e9), 709.9, -708.0,
                     np.nextafter(-708.0, -1e9), -745.0, -745.2, 1e300, -1e300, 0.5 * np.log(2.0), 1.5 * np.log(2.0), 5e-324, 1.0, -1.0])
    x = np.concatenate([rng.uniform(-760, 720, 400000), rng.normal(0, 3, 400000), 709.782712893384 + rng.uniform(-1e-9, 1e-9, 20000),
                        -708.0 + rng.uniform(-1e-9, 1e-9, 20000), edge])
    assert np.array_equal(_contract_eval(0, x, x.size), oracle.c_exp(x), equal_nan=True)
    xl = np.concatenate([np.exp(rng.uniform(-700, 700, 300000)), rng.random(100000), [0.0, 1.0, np.inf, 5e-324, 2.2250738585072014e-308, -1.0, np.nan]])
    assert np.array_equal(_contract_eval(1, xl, xl.size), oracle.c_log(xl), equal_nan=True)
    u = np.concatenate([(rng.integers(0, 2 ** 53, 300000).astype(np.float64) + 1.0) * 2.0 ** -53, [2.0 ** -53, 1.0, 0.5, 0.75, np.nextafter(1.0, 0)]])
    assert np.array_equal(_contract_eval(2, u, u.size), oracle.c_log_unit(u))
    v = np.concatenate([rng.random(300000), [0.0, 0.125, 0.25, 0.375, 0.5, 0.625, 0.75, 0.875, np.nextafter(1.0, 0)]])
    sc = _contract_eval(3, v, 2 * v.size).reshape(-1, 2)
    s_h, c_h = oracle.c_sincos2pi(v)
    assert np.array_equal(sc[:, 0], s_h) and np.array_equal(sc[:, 1], c_h)
    k24 = np.concatenate([rng.integers(0, 1 << 24, 400000), np.arange(0, 1 << 24, 1 << 16), np.arange(0, 1 << 24, 1 << 16) + 65535, [1, 2, (1 << 24) - 1]])
    sc = _contract_eval(6, k24.astype(np.float64), 2 * k24.size).reshape(-1, 2)
    s_h, c_h = oracle.c_sincos_u24(k24)
    assert np.array_equal(sc[:, 0], s_h) and np.array_equal(sc[:, 1], c_h)
    # the Box-Muller radius: the device's sqrt without the range handling its argument never needs == the host's IEEE sqrt, on
    # the arguments Box-Muller really produces (t = -2 log u1 over dense and extreme u1) and on dense samples of their range
    u1 = np.concatenate([(rng.integers(1, 2 ** 40, 2000000).astype(np.float64)) * 2.0 ** -40, np.arange(1, 200001) * 2.0 ** -40,
                         1.0 - np.arange(0, 200000) * 2.0 ** -40, [1.0, 2.0 ** -40]])
    tr = np.concatenate([-2.0 * oracle.c_log_unit(u1), np.exp(rng.uniform(np.log(2.0 ** -39), np.log(55.5), 2000000)), rng.uniform(0, 55.5, 1000000),
                         [0.0, -0.0, 2.0 ** -39, 55.5, 1.0, 4.0, 2.0, 0.25]])
    got = _contract_eval(7, tr, tr.size)
    assert np.array_equal(got.view(np.uint64), np.sqrt(tr).view(np.uint64))
    w = np.concatenate([rng.random(200000), rng.random(200000) * 2.0 ** -rng.integers(0, 1100, 200000), rng.random(1000) * 520, -rng.random(100),
                        [0.0, 1.0, 2.0 ** -96, 2.0 ** -97, 5e-324, 511.99999999999994, 512.0, np.inf, np.nan, 403.4287934927351]])
    fx = _contract_eval(4, w, 2 * w.size).view(np.uint64).reshape(-1, 2)
    assert np.array_equal(fx, oracle.c_fix(w))
    # the functions the samplers and the IF2 kernel evaluate per lane.  exp_le0: arguments <= 0 down to -745.2 and -inf, both sides of -708
    xe = np.concatenate([-rng.uniform(0, 745.2, 300000), -np.exp(rng.uniform(-700, 7, 100000)), -708.0 + rng.uniform(-1e-9, 1e-9, 20000),
                         [0.0, -0.0, 2.0 ** -20, -708.0, np.nextafter(-708.0, 0.0), np.nextafter(-708.0, -1e9), -745.0, -745.2, -1e300, -np.inf, -5e-324]])
    assert np.array_equal(_contract_eval(8, xe, xe.size).view(np.uint64), oracle.c_exp_le0(xe).view(np.uint64))
    # lgamma: (0, 24] dense (neighbouring lanes leave the recurrence loop after different trip counts), 24 .. 1e300, subnormal, and the NaN
    # of 0, negative and NaN arguments
    xg = np.concatenate([rng.uniform(0, 24, 400000), np.arange(1, 49) * 0.5, np.nextafter(np.arange(1.0, 25.0), 0.0), np.exp(rng.uniform(np.log(24.0), np.log(1e300), 200000)),
                         np.exp(rng.uniform(-745, 0, 100000)), [5e-324, 1e-310, 2.2250738585072014e-308, 24.0, 1e300, 2.0 ** 52 + 1.0,
                                                               0.0, -0.0, -1.0, -0.5, -np.inf, np.nan]])
    rng.shuffle(xg)
    got, want = _contract_eval(9, xg, xg.size), oracle.c_lgamma(xg)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isnan(want), ~(xg > 0.0))
    assert np.array_equal(got[xg > 0.0].view(np.uint64), want[xg > 0.0].view(np.uint64))
    # lgamma(k + 1): k = 0 .. 300 across the switch from the sum of logarithms to Stirling at 256, then large k
    kk = np.concatenate([np.arange(0, 301), rng.integers(0, 301, 2000), [1e6, 2.0 ** 31, 2.0 ** 52, 2.0 ** 52 - 1.0]]).astype(np.float64)
    assert np.array_equal(_contract_eval(10, kk, kk.size).view(np.uint64), oracle.c_lgamma_kp1(kk).view(np.uint64))
    for d in (1, 2, 3, 4, 9, 16):
        for first in (0, 7):   # even and odd first particle: both parities of the pair streams
            z = _contract_eval(5, np.array([cases.SEED, first, 3, 0, d], dtype=np.float64), 1001 * d).reshape(-1, d)
            np.testing.assert_array_equal(z, oracle.c_paired_normals(cases.SEED, first, 3, 0, d, 1001))


@pytest.mark.parametrize("sde", ["brownian", "gen_brownian", "ou"])
@pytest.mark.parametrize("obs", ["poisson", "linear"])
@pytest.mark.parametrize("n", [3000, (1 << 20) + 77])
def test_one_component_models_of_every_kind_bit_exact(sde, obs, n):
    """The six one-component structures k_propagate holds at compile time (cssm_prop.hip: KnownStructures<1> x Poisson / Gaussian
    observation), each in the single-tile kernel of a small cloud and in the whole-unit kernels of a large one, against the oracle
    (batch, with missing observations)."""
    from composablestatespacemodels_amd import Model, Parameters, Sde, SdeParameter
    sp = {"brownian": (Sde.brownianMotion(1), SdeParameter.brownianParameter(0.1, 1.0, 0.05)),
          "gen_brownian": (Sde.genBrownianMotion(1), SdeParameter.genBrownianParameter(0.1, 1.0, 0.02, 0.05)),
          "ou": (Sde.ouProcess(1), SdeParameter.ouParameter(0.1, 1.0, 0.3, 0.2, 0.2))}[sde]
    if obs == "poisson":
        model = Model.poisson(sp[0]).run(Parameters.apply(None, sp[1]))
        t, y, has = cases.poisson_counts(9, missing=0.2)
    else:
        model = Model.linear(sp[0]).run(Parameters.apply(np.log(0.5), sp[1]))
        t, y, has = cases.gaussian_series(9)
        has = np.ones(len(t), dtype=np.uint8); has[4] = 0
    g = NativePf(model, n, cases.SEED)
    o = oracle.OraclePf(model.descriptor(), n, cases.SEED)
    ll, ll_t, ess_t, _ = g.run(t, y, has)
    oll, oll_t, oess_t, _ = o.filter(t, y, has)
    assert ll == oll
    np.testing.assert_array_equal(ll_t, oll_t)
    np.testing.assert_array_equal(ess_t, oess_t)
    np.testing.assert_array_equal(g.particles(), o.particles())
    np.testing.assert_array_equal(g.ancestors(), o.ancestors())
    g.close()


OPT_WHOLE_TILES = 6   # CSSM_OPT_WHOLE_TILES: 1 / 2 / 3 = the launch geometries and kernels of clouds of 2^20 particles and more, at any size


@pytest.mark.parametrize("d", list(range(1, 17)))
def test_every_dimension_streaming_and_batch_bit_exact(d):
    """One k_propagate instantiation per latent dimension (particles per thread 2 / 1, 16- or 8-byte LDS staging, pair-shared
    normals for even IT) and launch geometry -- one tile per block (clouds below 2^20) and the three geometries of larger clouds,
    forced here: whole units with the single-tile-style kernel looping over their tiles, whole units with the software-pipelined
    kernel, one tile per block + k_reduce_units -- each against the oracle, with a ragged last tile."""
    model = cases.dim_model(d)
    assert model.descriptor().dim == d if hasattr(model.descriptor(), "dim") else True
    t, y, has = cases.poisson_counts(6, missing=0.2)
    _compare_streaming(model, 3001, t, y, has)
    n = 5 * 1024 + 77
    o = oracle.OraclePf(model.descriptor(), n, cases.SEED)
    ol, oll, oess, opath = o.filter(t, y, has, want_path=True)
    for whole in (0, 1, 2, 3):
        g = NativePf(model, n, cases.SEED)
        g.set_option(OPT_WHOLE_TILES, whole)
        assert g.d == d
        gl, gll, gess, gpath = g.run(t, y, has, want_path=True)
        assert gl == ol, (whole, gl, ol)
        np.testing.assert_array_equal(gess, oess)
        np.testing.assert_array_equal(gpath, opath)
        np.testing.assert_array_equal(g.ancestors(), o.ancestors())
        np.testing.assert_array_equal(g.particles(), o.particles())
        np.testing.assert_array_equal(g.proposed(), o.proposed())
        g.close()


OPT_GROUP_SUMS = 7    # CSSM_OPT_GROUP_SUMS: k_propagate's blocks also accumulate the sums of groups of 32 units, k_offspring reads those


@pytest.mark.parametrize("name,n,whole", [("c2_model", 100_000, 1), ("c2_model", 1 << 17, 2), ("c1_model", 65 * 1024 + 3, 1),
                                          ("c3_model", 64 * 1024, 1), ("c2_model", 70_001, 2)])
def test_group_sums_match_the_oracle_at_test_sizes(name, n, whole):
    """Scalars::grp (single GPU, one fused-sums block per unit, 64 units or more): k_propagate's blocks add the limbs of their unit
    sums to the sums of groups of 32 units with atomics, and every k_offspring block reads 32 group sums + the 32 unit sums of its
    own group instead of all unit sums.  Forced here at sizes the oracle finishes in seconds (whole units of 1024 particles: 64 to
    128 units, a partial last group, a ragged last unit), batch -- with a missing observation and, for c2, an outlying one that is
    redone relative to the max while the group sums of its first attempt stay behind -- and streaming, bit for bit; and the
    same handle with the option off."""
    model = getattr(cases, name)()
    t, y, has = cases.poisson_counts(9, missing=0.15)
    y = y.copy()
    if name == "c2_model":
        y[4] = 60.0; has[4] = 1      # an outlying observation (as _outlier_series): its reference level is ruled out by the max (redo_observation)
    o = oracle.OraclePf(model.descriptor(), n, cases.SEED)
    ol, oll, oess, _ = o.filter(t, y, has)
    for grp in (1, 0):
        g = NativePf(model, n, cases.SEED)
        g.set_option(OPT_WHOLE_TILES, whole); g.set_option(OPT_GROUP_SUMS, grp)
        for rep in range(2):                           # (the second run starts from the sets the first one left)
            gl, gll, gess, _ = g.run(t, y, has)
            assert gl == ol, (name, grp, rep, gl, ol)
            np.testing.assert_array_equal(gll, oll)
            np.testing.assert_array_equal(gess, oess)
            np.testing.assert_array_equal(g.ancestors(), o.ancestors())
            np.testing.assert_array_equal(g.particles(), o.particles())
        g.init(float(np.min(t)))
        o2 = oracle.OraclePf(model.descriptor(), n, cases.SEED); o2.init(float(np.min(t)))
        for s in range(6):
            assert g.step(t[s], y[s], bool(has[s])) == o2.step(t[s], y[s], bool(has[s])), (name, grp, s)
        np.testing.assert_array_equal(g.ancestors(), o2.ancestors())
        g.close()


@pytest.mark.parametrize("native_before", [1, 2, 4])
def test_group_sums_survive_a_host_resampled_step_in_between(native_before):
    """cssm_pf_propagate / cssm_pf_adopt (the host `Resample[A]` seam) between native fused steps: the seam restarts the rotation
    of max-slot / group-sum sets at 0, so it must leave every set clean -- with 1 (mod 3) native weighted steps before it, set 0
    still held the group sums of the last native step, and the next native step added its own on top (round 3's advisor:
    wrong S_tot and prefixes, silently).  70 units of 1024 particles, the group sums forced on; the host resampler hands back
    the oracle's resampled cloud, ll and ess, so every later native step must equal the oracle's bit for bit."""
    model = cases.c2_model()
    n = 70 * 1024 + 5
    T = native_before + 4
    t, y, has = cases.poisson_counts(T)
    g = NativePf(model, n, cases.SEED)
    g.set_option(OPT_WHOLE_TILES, 1); g.set_option(OPT_GROUP_SUMS, 1)
    o = oracle.OraclePf(model.descriptor(), n, cases.SEED)
    g.init(0.0); o.init(0.0)
    for s in range(T):
        ol, oe = o.step(t[s], y[s], True)
        if s in (native_before, native_before + 2):       # twice: the second time after two more native steps
            g.propagate(t[s], y[s], True)
            np.testing.assert_array_equal(g.proposed(), o.proposed())
            np.testing.assert_array_equal(g.logw(), o.logw())
            g.adopt(o.particles(), ol, oe)
        else:
            assert g.step(t[s], y[s], True) == (ol, oe), (native_before, s)
            np.testing.assert_array_equal(g.ancestors(), o.ancestors(), err_msg=f"step {s}")
        np.testing.assert_array_equal(g.particles(), o.particles(), err_msg=f"step {s}")
    # ... and a continued batch leg behind the seam (cssm_pf_ll_filter_more reads the same sets)
    t2, y2, has2 = cases.poisson_counts(T + 5)
    gl = g.run_more(t2[T:], y2[T:], has2[T:])[0]
    for s in range(T, T + 5):
        ol, oe = o.step(t2[s], y2[s], bool(has2[s]))
    assert gl == ol
    np.testing.assert_array_equal(g.ancestors(), o.ancestors())
    g.close()


@pytest.mark.parametrize("n", [1 << 20, (1 << 20) + 4097, 3 << 20, (5 << 20) + 1029, (1 << 23) + 5, 1 << 24])
def test_group_sums_on_and_off_agree_at_full_size(n, monkeypatch):
    """The same at the sizes where the group sums are the default (1024 units of 1024 .. 4096 particles, a ragged cloud whose last
    groups are short or empty; from 5 x 2^20 particles on units of 4 tiles -- 1281, 2049, 4096 of them -- whose sums k_offspring finds
    through up to 64 groups of 64 units, layout 2 of Scalars::grp): both settings of CSSM_OPT_GROUP_SUMS, and the units of the rule
    before round 5 (at most 1024 of them: CSSM_UNIT_MAX_TILES = 0), bit for bit, over a series with a missing observation."""
    model = cases.c2_model() if n not in ((1 << 23) + 5, 1 << 24) else cases.c1_model()
    t, y, has = cases.poisson_counts(7, missing=0.2)
    out = []
    for grp, old_units in ((1, False), (0, False), (1, True)):
        if old_units:
            monkeypatch.setenv("CSSM_UNIT_MAX_TILES", "0")
        g = NativePf(model, n, cases.SEED); g.set_option(OPT_GROUP_SUMS, grp)
        ll, llt, ess, _ = g.run(t, y, has)
        out.append((ll, llt, ess, g.ancestors(), g.particles())); g.close()
    for other in out[1:]:
        assert out[0][0] == other[0]
        for a, b in zip(out[0][1:], other[1:]):
            np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("name", ["c1", "c2", "c3", "linear", "negbin", "zip", "bernoulli", "studentt", "beta"])
def test_whole_tile_kernels_at_test_sizes(name):
    """The kernels large clouds run (CSSM_OPT_WHOLE_TILES = 1, 2, 3), every observation density, batch and streaming, with
    outliers absent and a missing observation -- against the oracle AND against the default single-tile path."""
    model, t, y, has = cases.golden_case(name, 12, missing=0.1)
    n = 3 * 1024 + 5
    o = oracle.OraclePf(model.descriptor(), n, cases.SEED)
    ol, oll, oess, _ = o.filter(t, y, has)
    for whole in (1, 2, 3, 0):
        g = NativePf(model, n, cases.SEED)
        g.set_option(OPT_WHOLE_TILES, whole)
        gl, gll, gess, _ = g.run(t, y, has)
        assert gl == ol, (name, whole)
        np.testing.assert_array_equal(gll, oll)
        np.testing.assert_array_equal(gess, oess)
        np.testing.assert_array_equal(g.ancestors(), o.ancestors())
        _assert_weights_match(g, o.logw(), o) if has[-1] else None
        g.init(float(np.min(t)))                       # the same handle, streaming, same geometry
        o2 = oracle.OraclePf(model.descriptor(), n, cases.SEED); o2.init(float(np.min(t)))
        for s in range(4):
            assert g.step(t[s], y[s], bool(has[s])) == o2.step(t[s], y[s], bool(has[s]))
        np.testing.assert_array_equal(g.particles(), o2.particles())
        g.close()


# ----------------------------------------------------------------------------- tolerance to the reference's literal arithmetic
# The north star asks for the marginal log-likelihood "to a stated fp64 tolerance" of the reference CPU filter.  The closest
# executable form of the reference's own arithmetic is the oracle in LITERAL_SUMS | LIBM mode: sequential fp64 sums and
# cumulative weights (Seq.sum / scanLeft, model/ParticleFilter.scala:124-128, model/Resampling.scala:21-24,57), the platform
# libm instead of the contract's elementary functions, rescaling by the max.  The stated tolerance (DESIGN.md section 2,
# include/cssm_pf.h):  |ll_HIP - ll_literal| <= LL_TOL_PER_OBS * T, and no more than FLIPPED_ANCESTORS_MAX of the ancestor
# indices of the first weighted observation differ (measured: none).
# TIE_LAST adds the TreeMap quirk (:57: equal consecutive cumulative weights are ONE key whose value is the LAST particle
# inserted).  At large N that is no corner case: a weight below half an ulp of the running cumulative sum leaves the sum
# unchanged, so a particle of negligible weight takes the slot of the heavy particle before it (0.4 % of the slots at
# N = 2^16 on the bench model).  The contract keeps the first particle (deviation D3) -- the one that owns the probability
# mass.  One such swap changes the later cumulative weights by O(1/N), i.e. by a fraction of a slot, so from the next
# observation on the two runs are different realisations of the same estimator: the test pins (i) that EVERY differing
# ancestor of the first weighted observation is such a swap and (ii) agreement of ll within Monte-Carlo error.
LL_TOL_PER_OBS = 1e-9
FLIPPED_ANCESTORS_MAX = 1e-4     # fraction of slots whose ancestor may differ after the FIRST weighted observation


@pytest.mark.parametrize("name,n,T", [("c1_model", 1000, 100), ("c2_model", 1 << 16, 60),
                                      # round 4: the widest bench model (d = 9), the LGCP filter (precision 2: sub-steps, hazard sums, levels predicted
                                      # from the previous event's max against the reference's plain max) and a "next" density (negative binomial)
                                      ("c3_model", 1 << 14, 40), ("c4_model", 1 << 14, 25), ("negbin_model", 1 << 15, 40)])
def test_hip_likelihood_within_stated_tolerance_of_literal_reference_arithmetic(name, n, T):
    model = getattr(cases, name)()
    prec = 2 if name == "c4_model" else 0
    t, y, has = cases.event_times(T, horizon=0.1 * T) if prec else cases.poisson_counts(T)
    g = NativePf(model, n, cases.SEED, lgcp_precision=prec)
    gl, gl_t, gess, _ = g.run(t, y, has)
    t0 = float(np.min(t))
    s0 = int(np.argmax(has))

    def first_weighted_step(flags):
        g.init(t0)
        o = oracle.OraclePf(model.descriptor(prec), n, cases.SEED, flags)
        o.init(t0)
        for s in range(s0 + 1):
            g.step(t[s], y[s], bool(has[s])); o.step(t[s], y[s], bool(has[s]))
        return g.ancestors().astype(np.int64), o.ancestors().astype(np.int64), o.logw()

    # (a) literal sums + libm: the stated tolerance
    flags = oracle.LITERAL_SUMS | oracle.LIBM
    ol, ol_t, oess, _ = oracle.OraclePf(model.descriptor(prec), n, cases.SEED, flags).filter(t, y, has)
    assert abs(gl - ol) <= LL_TOL_PER_OBS * T, (gl, ol)
    assert np.max(np.abs(gl_t - ol_t)) <= LL_TOL_PER_OBS * T
    assert np.max(np.abs(gess.astype(np.int64) - oess.astype(np.int64))) <= 1
    ga, oa, _ = first_weighted_step(flags)
    flipped = float(np.mean(ga != oa))
    assert flipped <= FLIPPED_ANCESTORS_MAX
    # (b) ... + the TreeMap duplicate-key quirk
    flags |= oracle.TIE_LAST
    tl = oracle.OraclePf(model.descriptor(prec), n, cases.SEED, flags).filter(t, y, has)[0]
    ga, oa, lw = first_weighted_step(flags)
    diff = np.nonzero(ga != oa)[0]
    w1 = np.exp(lw - lw.max())
    rel = w1 / w1.sum()
    for i in diff:
        assert oa[i] > ga[i]                                   # the reference's key maps to a LATER particle ...
        assert rel[ga[i] + 1:oa[i] + 1].max() <= 2.0 ** -52    # ... and everything up to it is too light to move the cumulative sum
    assert abs(gl - tl) <= 0.25                                # different realisations from here on: Monte-Carlo agreement only
    print(f"{name} N={n} T={T}: |dll| literal+libm = {abs(gl - ol):.3e} (tolerance {LL_TOL_PER_OBS * T:.1e}), flipped ancestors {flipped:.1e}; "
          f"with TreeMap last-wins ties: {len(diff) / n:.2e} of the first observation's slots swap to a negligible particle, |dll| = {abs(gl - tl):.3e}")
    g.close()


def test_set_params_is_transactional_and_keeps_the_structure():
    """A failing cssm_pf_set_params leaves the handle's previous parameters in force, whole; a descriptor of another model
    structure (or observation model) is refused instead of silently re-purposing the handle."""
    from composablestatespacemodels_amd._abi import CssmError
    t, y, has = cases.poisson_counts(6)
    g = NativePf(cases.c2_model(), 2000, cases.SEED)
    ll0 = g.run(t, y, has)[0]
    with pytest.raises(CssmError):
        g.set_params(cases.c3_model())            # other leaves / dimension
    with pytest.raises(CssmError):
        g.set_params(cases.c1_model())
    with pytest.raises(CssmError):
        g.set_params(cases.linear_model())        # other observation model
    assert g.run(t, y, has)[0] == ll0             # nothing of the rejected descriptors stuck
    g.set_params(cases.c2_model())                # the same structure is accepted
    assert g.run(t, y, has)[0] == ll0
    g.close()


def test_filter_with_a_host_resample_function():
    """`Filter(mod, f)` for an arbitrary `Resample[A]` (model/package.scala:23): the device propagates and weighs, the function
    resamples on the host.  (i) a host restatement of systematic resampling driven by the contract's own uniform reproduces
    the native filter bit for bit -- particles, ess; ll to the last bits (the host sums in plain fp64); (ii) Resampling.indentity
    (model/Resampling.scala:29) leaves the cloud unresampled: ll and ess still follow :127-128."""
    from composablestatespacemodels_amd.filter import Filter
    from composablestatespacemodels_amd.model import TimedObservation
    model = cases.c2_model()
    n, T = 4000, 6
    t, y, has = cases.poisson_counts(T, missing=0.2)
    data = [TimedObservation(float(a), float(b) if h else None) for a, b, h in zip(t, y, has)]
    step = {"s": 0}

    def host_systematic(particles, w1):
        # the contract's ancestors for these weights and this observation's uniform (cssm_resample_systematic with the
        # same u the native filter draws: stream U, observation index)
        u = float(oracle.lib().oracle_c_u(cases.SEED, step["s"]))
        anc = Resampling.systematicAncestors(w1, u)
        return [particles[int(a)] for a in anc]

    f = Filter(model, host_systematic, seed=cases.SEED)
    g = Filter(model, Resampling.systematicResampling, seed=cases.SEED)
    sf, sg = f.initialiseState(n, 0.0), g.initialiseState(n, 0.0)
    for k, d in enumerate(data):
        step["s"] = k
        sf, sg = f.stepFilter(sf, d), g.stepFilter(sg, d)
        np.testing.assert_array_equal(sf.particles, sg.particles)
        assert sf.ess == sg.ess and abs(sf.ll - sg.ll) < 1e-9
    # identity: no resampling at all
    fi = Filter(model, Resampling.indentity, seed=cases.SEED)
    si = fi.initialiseState(n, 0.0)
    o = oracle.OraclePf(model.descriptor(), n, cases.SEED)
    o.init(0.0)
    o.propagate_only(data[0].t, data[0].observation, True)
    si = fi.stepFilter(si, data[0])
    np.testing.assert_array_equal(si.particles, o.proposed())          # the proposed cloud, unresampled
    w = o.logw(); w1 = np.exp(w - w.max())
    assert abs(si.ll - (w.max() + np.log(w1.sum() / n))) < 1e-12 and si.ess == int(np.floor(1.0 / np.sum((w1 / w1.sum()) ** 2)))
    assert fi.llFilter(data, n) == fi.llFilter(data, n)                # deterministic under the handle's seed


@pytest.mark.parametrize("name,n,T,lgcp", [("c3_model", 1 << 22, 4, 0), ("c4_model", 1 << 24, 3, 2), ("c2_model", 100_000, 6, 0),
                                           # the launch geometries of the large clouds at sizes where they are the default: whole units of
                                           # 3 and 4 tiles of 1024 looped over (odd unit size; the 8-tile limit), the software-pipelined
                                           # kernel beyond it (ragged N), one tile per block + k_reduce_units for a wide state (ragged N)
                                           ("c2_model", 3 << 20, 3, 0), ("c2_model", 1 << 22, 3, 0), ("c1_model", (1 << 23) + 5, 3, 0),
                                           ("max_dim_model", (1 << 21) + 77, 3, 0)])
def test_full_size_configs_oracle_checked_on_slices(name, n, T, lgcp):
    """BASELINE configs 3 (d = 9, N = 2^22), 4 (LGCP, N = 2^24) and 5's filter (N = 100 000) at their FULL particle counts, checked
    against the oracle where the one-thread oracle can go: slices of the cloud.  Variates are keyed by the global particle id,
    so an oracle shard [first, first + m) of an N-particle filter, handed the GPU's resampled cloud of its slice, must
    reproduce the GPU's propagated particles and log-weights of that slice bit for bit at every observation (the initial
    cloud included) -- three slices per configuration, one with an odd start (unpaired normal streams).  The resampling
    in between is global; the offspring-count property of test_full_size_c3_c4_size_independent_properties pins it."""
    model = getattr(cases, name)()
    t, y, has = (cases.event_times(T) if lgcp else cases.poisson_counts(T, missing=0.25))
    g = NativePf(model, n, cases.SEED, lgcp_precision=lgcp)
    t0 = float(np.min(t))
    g.init(t0)
    slices = [(0, 4096), (n // 2 - 1001, 4097), (n - 3000, 3000)]
    shards = []
    cloud = g.particles()
    for first, m in slices:
        o = oracle.OraclePf(model.descriptor(lgcp), m, cases.SEED)
        o.set_shard(first, n)
        o.init(t0)
        np.testing.assert_array_equal(o.particles(), cloud[:, first:first + m], err_msg=f"initial cloud, slice at {first}")
        shards.append(o)
    for s in range(T):
        g.step(t[s], y[s], bool(has[s]))
        prop = g.proposed()
        for (first, m), o in zip(slices, shards):
            o.set_particles(np.ascontiguousarray(cloud[:, first:first + m]))
            o.propagate_only(float(t[s]), float(y[s]), bool(has[s]))
            np.testing.assert_array_equal(o.proposed(), prop[:, first:first + m], err_msg=f"step {s}, slice at {first}: propagated cloud")
            if has[s] or lgcp:
                kept = g.weights()
                if kept is None:
                    np.testing.assert_array_equal(o.logw(), g.logw()[first:first + m], err_msg=f"step {s}, slice at {first}: log-weights")
                else:
                    olw = np.where(np.isnan(o.logw()), -np.inf, o.logw())
                    np.testing.assert_array_equal(oracle.c_exp(np.minimum(olw - kept[1], 2.0 ** -20)), kept[0][first:first + m],
                                                  err_msg=f"step {s}, slice at {first}: weights")
        cloud = g.particles()
    g.close()


# ----------------------------------------------------------------------------- continuing a batch run
@pytest.mark.parametrize("name,n,whole,kind", [("c2_model", 3000, 0, 0), ("c2_model", 5 * 1024 + 3, 1, 0), ("c3_model", 4096, 0, 0),
                                               ("c3_model", 3 * 1024, 1, 0), ("c1_model", 1000, 2, 0), ("linear_model", 2500, 0, 0),
                                               ("c2_model", 2500, 0, 1), ("c2_model", 2500, 0, 2), ("c3_model", 5 * 1024 + 9, 3, 0), ("c2_model", 4 * 1024 + 1, 3, 0)])
def test_ll_filter_more_continues_the_series_bit_for_bit(name, n, whole, kind):
    """cssm_pf_ll_filter(t[:a]) then cssm_pf_ll_filter_more(t[a:b]), (t[b:]) = cssm_pf_ll_filter(t) = the oracle: ll, ll_t, ess_t,
    ancestors, clouds -- with missing observations, outlying observations in the continued parts (held and redone with the
    call's own record indices), in every launch geometry and with every native resampler (whose per-observation variates are
    keyed by the observation's index in the FILTER's series)."""
    model = getattr(cases, name)()
    t, y, has = cases.poisson_counts(26, missing=0.15)
    y = y.copy()
    if name != "linear_model":
        y[11] = 70.0; y[12] = 85.0; y[25] = 95.0; has[11] = has[12] = has[25] = 1
    a, b = 9, 12
    g = NativePf(model, n, cases.SEED); g.set_option(OPT_WHOLE_TILES, whole); g.set_option(2, kind)
    g.run(t[:a], y[:a], has[:a])
    l1 = g.run_more(t[a:b], y[a:b], has[a:b])
    l2 = g.run_more(t[b:], y[b:], has[b:])
    f = NativePf(model, n, cases.SEED); f.set_option(OPT_WHOLE_TILES, whole); f.set_option(2, kind)
    fl, fll, fess, _ = f.run(t, y, has)
    assert l2[0] == fl
    np.testing.assert_array_equal(np.concatenate([l1[1], l2[1]]), fll[a:])
    np.testing.assert_array_equal(np.concatenate([l1[2], l2[2]]), fess[a:])
    np.testing.assert_array_equal(g.ancestors(), f.ancestors())
    np.testing.assert_array_equal(g.particles(), f.particles())
    np.testing.assert_array_equal(g.proposed(), f.proposed())
    if kind == 0:
        o = oracle.OraclePf(model.descriptor(), n, cases.SEED)
        ol = o.filter(t, y, has)[0]
        assert l2[0] == ol
        np.testing.assert_array_equal(g.particles(), o.particles())
    # ... and streaming steps continue from there
    gs = g.step(27.0, 3.0, True); fs = f.step(27.0, 3.0, True)
    assert gs == fs
    g.close(); f.close()


def test_ll_filter_more_needs_a_running_filter():
    g = NativePf(cases.c1_model(), 100, 1)
    with pytest.raises(Exception):
        g.run_more(np.array([1.0]), np.array([1.0]))
    g.close()


@pytest.mark.gpu
def test_records_sent_by_kernel_or_by_copy_give_the_same_series():
    """The observation records reach the device through k_fetch_recs (a kernel reading the pinned host buffer, the first record of a
    continued call ahead of the rest) or, with CSSM_UPLOAD_MEMCPY=1, through hipMemcpyAsync as in rounds 1-3: the same bits either way
    (a child process per setting: the library reads the variable once)."""
    import json, os, subprocess, sys
    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = (
        "import sys, json, hashlib; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "import numpy as np, cases\n"
        "from composablestatespacemodels_amd.filter import NativePf\n"
        "t, y, has = cases.poisson_counts(40, missing=0.1)\n"
        "g = NativePf(cases.c2_model(), 6000, cases.SEED)\n"
        "a = g.run(t[:7], y[:7], has[:7]); b = g.run_more(t[7:30], y[7:30], has[7:30]); c = g.run_more(t[30:], y[30:], has[30:])\n"
        "s = g.step(41.0, 2.0, True)\n"
        "h = hashlib.sha256(); [h.update(np.ascontiguousarray(x).tobytes()) for x in (b[1], b[2], c[1], c[2], g.ancestors(), g.particles())]\n"
        "print(json.dumps({'ll': [a[0], b[0], c[0], s[0]], 'digest': h.hexdigest()}))\n"
    ) % (ROOT, os.path.join(ROOT, "tests"))
    outs = []
    for extra in ({}, {"CSSM_UPLOAD_MEMCPY": "1"}):
        env = dict(os.environ); env.pop("CSSM_UPLOAD_MEMCPY", None); env.update(extra)
        r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        outs.append(json.loads(r.stdout.strip().splitlines()[-1]))
    assert outs[0] == outs[1]
