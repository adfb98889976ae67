"""cssm_pf_filter_forecasts / _more / cssm_pf_step_forecast (include/cssm_pf.h; csrc/cssm_intervals.hip, k_forecast_row in
csrc/cssm_forecast.hip): the one-step-ahead forecasts of one cloud, a row per record from the batch call, formed before the record is
weighed.  The reference of every row is the route the library had before: a second handle of the same seed driven through
forecast([t_s], key_s); step(...) per record, its PIT counts counted with numpy from forecast(..., want_samples=True)'s observation row.
Everything is compared with assert_array_equal -- order statistics AND means --, the filter's results with run / run_more, and the
handles afterwards as test_gpu_filter_intervals.same_handles does."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import cases
from composablestatespacemodels_amd import CssmError, Data, _abi
from composablestatespacemodels_amd.filter import FORECAST_NAMES, Filter, NativePf, ParticleFilter, Resampling
from composablestatespacemodels_amd.formats import forecast_out_csv
from test_filter_forecasts_host import run_key
from test_gpu_filter_intervals import MODELS, same_handles, series
from test_gpu_forecast import beta_scaled_model

pytestmark = pytest.mark.gpu
SEED = cases.SEED
KEY = 0x0E57E9F0CA57
PIT = ("obs_below", "obs_equal")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def loop_rows(g: NativePf, t, y, has, keys=None, interval=0.975, init=True):
    """The route before this call existed, on the handle g: per record forecast([t_s], key_s, want_samples=True), then step.  The dict
    filter_forecasts returns; a record whose time forecast refuses keeps its NaN row and counts of -1."""
    T, d = len(t), g.d
    if init:
        g.init(float(np.min(t)))
    out = {k: np.full((T, d) if k.startswith("state") else T, np.nan) for k in FORECAST_NAMES}
    out.update({k: np.full(T, -1, dtype=np.int32) for k in PIT})
    ll_t, ess_t, used = [], [], []
    for s in range(T):
        key = g.forecast_key() if keys is None else int(keys[s])
        used.append(key)
        try:
            r = g.forecast([float(t[s])], key, interval, want_samples=True)
        except CssmError:
            r = None
        if r is not None:
            for k in FORECAST_NAMES:
                out[k][s] = r[k][0]
            if has[s]:
                obs = r["samples"][0][d + 2]
                out["obs_below"][s] = int(np.sum(obs < y[s])); out["obs_equal"][s] = int(np.sum(obs == y[s]))
        ll, ess = g.step(float(t[s]), float(y[s]), bool(has[s]))
        ll_t.append(ll); ess_t.append(ess)
    out.update(ll=ll_t[-1], ll_t=np.array(ll_t), ess_t=np.array(ess_t, dtype=np.int32), keys=np.array(used, dtype=np.uint64))
    return out


def same_rows(got, want, what=""):
    assert got["ll"] == want["ll"], what
    for k in ("ll_t", "ess_t", "keys") + FORECAST_NAMES + PIT:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, (what, k)
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"{what} {k}")


def both_routes(model, n, t, y, has, keys=None, interval=0.975, option=None, t_next=None, check_run=True):
    with NativePf(model, n, SEED) as a, NativePf(model, n, SEED) as b:
        if option is not None:
            a.set_option(*option); b.set_option(*option)
        got = a.filter_forecasts(t, y, has, keys, interval)
        want = loop_rows(b, t, y, has, keys, interval)
        same_rows(got, want, f"n={n}")
        same_handles(a, b, float(t[-1]) + 1.0 if t_next is None else t_next, f"n={n}")
    if check_run:                                                           # the filter's results: cssm_pf_ll_filter's
        with NativePf(model, n, SEED) as c:
            if option is not None:
                c.set_option(*option)
            ll, ll_t, ess_t, _ = c.run(t, y, has)
        assert got["ll"] == ll
        np.testing.assert_array_equal(got["ll_t"], ll_t); np.testing.assert_array_equal(got["ess_t"], ess_t)
    return got


# 1 ------------------------------------------------------------------------------------------------------------------------------
# 511 / 512 / 513: the block edge of the pair kernel (256 threads x 2 particles); 4097: above CSSM_IV_CAP; 131073 (c2 only): 65537 pairs =
# 257 blocks of k_forecast_row, the smallest cloud at which the block-strided loops of k_fc_finish (partial sums, PIT counts) and of the
# selection's first derivation take a second turn -- the clearing loop of k_forecast_row takes several at every smaller size
SMALL = [1, 2, 3, 63, 64, 65, 511, 512, 513, 1000, 4097]


@pytest.mark.parametrize("name,n", [(name, n) for name in MODELS for n in SMALL] + [("c2", 131073)])
def test_rows_equal_the_forecast_then_step_loop(name, n):
    t, y, has = series()
    got = both_routes(MODELS[name](), n, t, y, has)
    d = MODELS[name]().dimension
    assert got["state_mean"].shape == (12, d) and got["obs_mean"].shape == (12,)
    assert got["obs_below"][3] == -1 and got["obs_equal"][3] == -1          # record 3 has no datum
    assert np.isfinite(got["obs_mean"]).all()


# 2 ------------------------------------------------------------------------------------------------------------------------------
SAMPLERS = {"linear": lambda: cases.literal_case("linear", 10), "negbin": lambda: cases.literal_case("negbin", 10),
            "zip": lambda: cases.literal_case("zip", 10), "bernoulli": lambda: cases.literal_case("bernoulli", 10),
            "studentt": lambda: cases.literal_case("studentt", 10), "euler": lambda: cases.literal_case("euler", 10),
            "beta": lambda: (beta_scaled_model(),) + tuple(cases.unit_interval_series(10))}


@pytest.mark.parametrize("name", list(SAMPLERS))
def test_every_observation_sampler(name):
    """Bernoulli and ZIP: the tie-heavy observation rows.  (Beta: cases.beta_model carries no shape, so its observation cannot be drawn --
    that model is the refusal of test_refusals_by_code_and_message; the sampler runs here on the same model with its shape given.)"""
    model, t, y, has = SAMPLERS[name]()
    got = both_routes(model, 1000, t, y, has)
    if name in ("bernoulli", "zip"):
        assert (got["obs_equal"][np.asarray(has, bool)] > 0).any()


# 3 ------------------------------------------------------------------------------------------------------------------------------
def test_default_keys_and_given_keys():
    model, n = cases.c2_model(), 1000
    t, y, has = series()
    got = both_routes(model, n, t, y, has, keys=None, check_run=False)
    np.testing.assert_array_equal(got["keys"], np.array([run_key(SEED, s) for s in range(12)], dtype=np.uint64))
    keys = [run_key(KEY, 7 * s + 1) for s in range(12)]
    given = both_routes(model, n, t, y, has, keys=keys, check_run=False)
    assert not np.array_equal(given["obs_mean"], got["obs_mean"])
    for k in ("ll_t", "ess_t"):                                             # the keys move the forecasts, not the filter
        np.testing.assert_array_equal(given[k], got[k])


# 4 ------------------------------------------------------------------------------------------------------------------------------
def test_a_held_and_redone_observation():
    """The fixture of test_gpu_filter_intervals.test_a_held_and_redone_observation: the series is put on hold at record 5.  Its own row was
    formed before the hold and stands; the rows behind it returned at once and are formed with the records enqueued again."""
    t, y, has = cases.poisson_counts(9, missing=0.2)
    y = y.copy(); y[5] = 70.0; has = has.copy(); has[5] = 1
    both_routes(cases.c2_model(), 4096, t, y, has)
    with NativePf(cases.c2_model(), 4096, SEED) as a, NativePf(cases.c2_model(), 4096, SEED) as b:   # ... and inside a continued call
        a.init(0.0); b.init(0.0)
        got = a.filter_forecasts_more(t, y, has)
        want = loop_rows(b, t, y, has, init=False)
        same_rows(got, want, "continued")
        same_handles(a, b, 10.0, "continued")
    with NativePf(cases.c2_model(), 4096, SEED) as a, NativePf(cases.c2_model(), 4096, SEED) as b:   # ... and in the stream (the redo inside the step)
        a.init(0.0); b.init(0.0)
        rows = [a.step_forecast(float(t[s]), float(y[s]), bool(has[s])) for s in range(len(t))]
        want = loop_rows(b, t, y, has, init=False)
        np.testing.assert_array_equal(np.array([r[0] for r in rows]), want["ll_t"])
        np.testing.assert_array_equal(np.array([r[1] for r in rows], dtype=np.int32), want["ess_t"])
        for k in FORECAST_NAMES + PIT:
            np.testing.assert_array_equal(np.concatenate([r[2][k] for r in rows]), want[k], err_msg=f"stream {k}")
        same_handles(a, b, 10.0, "stream")


# 5 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("resampler", [1, 2])                                # stratified; multinomial (ancestors not sorted: the other gather pattern)
def test_stratified_and_multinomial_resamplers(resampler):
    t, y, has = series()
    both_routes(cases.c2_model(), 1000, t, y, has, option=(2, resampler))   # CSSM_OPT_RESAMPLER


# 6 ------------------------------------------------------------------------------------------------------------------------------
SWITCHES = [(3, 0), (6, 1), (10, 2), (2, 1), (3, 1), (6, 0), (2, 0), (10, 0)]   # CSSM_OPT_FUSED_SUMS, _WHOLE_TILES, _WAVE_SUMS, _RESAMPLER


def test_stream_and_continued_calls_with_option_switches_between_them():
    model, n = cases.c2_model(), 1000
    t, y, has = series()
    with NativePf(model, n, SEED) as g:
        whole = g.filter_forecasts(t, y, has, None, 0.9)
        ms = g.forecasts_last_ms()
        assert len(ms) == 2 and all(math.isfinite(v) and v > 0.0 for v in ms), ms
    with NativePf(model, n, SEED) as g:                                     # filter_forecasts(t[:5]) then _more(t[5:]) = one call over all records
        a = g.filter_forecasts(t[:5], y[:5], has[:5], None, 0.9)
        b = g.filter_forecasts_more(t[5:], y[5:], has[5:], None, 0.9)
    assert b["ll"] == whole["ll"]
    for k in ("ll_t", "ess_t", "keys") + FORECAST_NAMES + PIT:
        np.testing.assert_array_equal(np.concatenate([a[k], b[k]]), whole[k], err_msg=k)
    with NativePf(model, n, SEED) as g:                                     # the stream: step_forecast per record
        g.init(float(np.min(t)))
        rows = [g.step_forecast(float(t[s]), float(y[s]), bool(has[s]), None, 0.9) for s in range(len(t))]
        ms = g.forecasts_last_ms()
        assert all(math.isfinite(v) and v > 0.0 for v in ms), ms
    np.testing.assert_array_equal(np.array([r[0] for r in rows]), whole["ll_t"])
    np.testing.assert_array_equal(np.array([r[1] for r in rows], dtype=np.int32), whole["ess_t"])
    for k in FORECAST_NAMES + PIT:
        np.testing.assert_array_equal(np.concatenate([r[2][k] for r in rows]), whole[k], err_msg=f"stream {k}")
    assert [r[2]["key"] for r in rows] == [int(v) for v in whole["keys"]]
    # the switches change the source the next row reads (src, anc_valid, the split source), never a bit: the systematic ones against
    # `whole`, a resampler switch against the loop under the same switches
    with NativePf(model, n, SEED) as g, NativePf(model, n, SEED) as ref:
        g.init(float(np.min(t))); ref.init(float(np.min(t)))
        got, want = [], []
        for s in range(len(t)):
            g.set_option(*SWITCHES[s % len(SWITCHES)]); ref.set_option(*SWITCHES[s % len(SWITCHES)])
            if s % 3 == 2:
                ll, ess, fc = g.step_forecast(float(t[s]), float(y[s]), bool(has[s]), None, 0.9)
                got.append({**fc, "ll_t": np.array([ll]), "ess_t": np.array([ess], dtype=np.int32), "keys": np.array([fc["key"]], dtype=np.uint64), "ll": ll})
            else:
                got.append(g.filter_forecasts_more(t[s:s + 1], y[s:s + 1], has[s:s + 1], None, 0.9))
            want.append(loop_rows(ref, t[s:s + 1], y[s:s + 1], has[s:s + 1], None, 0.9, init=False))
        for k in ("ll_t", "ess_t", "keys") + FORECAST_NAMES + PIT:
            np.testing.assert_array_equal(np.concatenate([r[k] for r in got]), np.concatenate([r[k] for r in want]), err_msg=f"switched {k}")
        same_handles(g, ref, float(t[-1]) + 1.0, "switched")
    with NativePf(model, n, SEED) as g:                                     # without a resampler switch the bits are those of the plain call
        for s0, (opt, val) in zip(range(0, 12, 3), [(3, 0), (6, 1), (10, 2), (3, 1)]):
            g.set_option(opt, val)
            fn = g.filter_forecasts if s0 == 0 else g.filter_forecasts_more
            r = fn(t[s0:s0 + 3], y[s0:s0 + 3], has[s0:s0 + 3], None, 0.9)
            for k in ("ll_t", "ess_t", "keys") + FORECAST_NAMES + PIT:
                np.testing.assert_array_equal(r[k], whole[k][s0:s0 + 3], err_msg=f"systematic switches {k} from {s0}")


# 7 ------------------------------------------------------------------------------------------------------------------------------
def test_a_collapsed_cloud_from_the_filter_itself():
    """A Gaussian observation with a tiny scale leaves ESS = 1: the next row moves N copies of one particle, reached through the ancestors."""
    model, n = cases.linear_model(obs_sd=1e-7), 4097
    t, y, has = np.array([0.0, 1.0, 2.0]), np.array([0.4, 0.45, 0.5]), np.ones(3, dtype=np.uint8)
    got = both_routes(model, n, t, y, has)
    assert got["ess_t"][0] == 1, got["ess_t"]


# 8 ------------------------------------------------------------------------------------------------------------------------------
def _outcome(call):
    try:
        return "ok", call()
    except CssmError as e:
        return "error", e.code


def test_a_refused_time_reads_a_nan_row():
    """A record that lies before the clock the record before it left: cssm_pf_forecast refuses that time from that cloud, so its row is
    NaN / -1 while the rows before it are the loop's; the filter part does with the record what cssm_pf_ll_filter does.  As the last
    record and without a datum nothing is weighed behind it: both routes return, and the call's results are run's.  In the middle of a
    series the filter part's outcome -- the error code, if the backward step breaks the cloud -- is run's as well."""
    model, n = cases.c2_model(), 1000
    t, y, has = series()
    t = t.copy(); t[11] = t[10] - 0.5; has = has.copy(); has[11] = 0
    with NativePf(model, n, SEED) as a, NativePf(model, n, SEED) as b, NativePf(model, n, SEED) as c:
        got = a.filter_forecasts(t, y, has)
        want = loop_rows(b, t, y, has)
        same_rows(got, want, "refused last")
        ll, ll_t, ess_t, _ = c.run(t, y, has)
        assert got["ll"] == ll
        np.testing.assert_array_equal(got["ll_t"], ll_t); np.testing.assert_array_equal(got["ess_t"], ess_t)
        for p in (b, c):
            np.testing.assert_array_equal(a.particles(), p.particles()); np.testing.assert_array_equal(a.ancestors(), p.ancestors())
            assert a.observation_index() == p.observation_index() == 12
    for k in FORECAST_NAMES:
        assert np.isnan(got[k][11]).all(), k
        assert np.isfinite(got[k][:11]).all(), k
    assert got["obs_below"][11] == -1 and got["obs_equal"][11] == -1
    t2, y2, has2 = series()
    t2 = t2.copy(); t2[4] = t2[3] - 0.5                                      # ... in the middle, weighted records behind it
    with NativePf(model, n, SEED) as a, NativePf(model, n, SEED) as c:
        ra, rc_ = _outcome(lambda: a.filter_forecasts(t2, y2, has2)), _outcome(lambda: c.run(t2, y2, has2))
        assert ra[0] == rc_[0]
        if ra[0] == "error":
            assert ra[1] == rc_[1]
        else:
            assert ra[1]["ll"] == rc_[1][0] and np.isnan(ra[1]["obs_mean"][4]) and ra[1]["obs_below"][4] == -1
            np.testing.assert_array_equal(ra[1]["ll_t"], rc_[1][1])
    with NativePf(model, n, SEED) as a, NativePf(model, n, SEED) as b:      # ... and in the stream, on a record without a datum
        a.init(2.0); b.init(2.0)
        ll, ess, fc = a.step_forecast(1.0, None)
        assert (ll, ess) == b.step(1.0, None)
        assert all(np.isnan(fc[k]).all() for k in FORECAST_NAMES) and fc["obs_below"][0] == -1 and fc["obs_equal"][0] == -1
        np.testing.assert_array_equal(a.particles(), b.particles())


# 9 ------------------------------------------------------------------------------------------------------------------------------
def test_filter_forecasts_writes_the_lines_of_getmeanforecast_then_stepfilter(tmp_path):
    model, n = cases.c2_model(), 1000
    t, y, has = series()
    data = [Data(float(a), float(b) if h else None) for a, b, h in zip(t, y, has)]
    ll, outs = Filter(model, Resampling.systematicResampling, seed=SEED).filterForecasts(data, n, 0.9)
    flt = Filter(model, Resampling.systematicResampling, seed=SEED)
    s = flt.initialiseState(n, float(np.min(t)))
    want = []
    for dd in data:
        want.append(ParticleFilter.getMeanForecast(s, model, dd.t, 0.9))
        s = flt.stepFilter(s, dd)
    assert ll == s.ll and len(outs) == len(data) and [o.t for o in outs] == [dd.t for dd in data]
    assert [forecast_out_csv(o) for o in outs] == [forecast_out_csv(o) for o in want]
    f2 = Filter(model, Resampling.systematicResampling, seed=SEED)         # stepForecast: the stream with its ForecastOut per element
    s2 = f2.initialiseState(n, float(np.min(t)))
    lines = []
    for dd in data:
        s2, out = f2.stepForecast(s2, dd, 0.9)
        lines.append(forecast_out_csv(out))
    assert s2.ll == ll and lines == [forecast_out_csv(o) for o in want]
    # a host Resample[A] has no batch path: the loop of getMeanForecast then stepFilter
    fh = Filter(model, Resampling.residualResampling, seed=SEED)
    llh, outh = fh.filterForecasts(data[:4], 200, 0.9)
    assert len(outh) == 4 and math.isfinite(llh) and [o.t for o in outh] == [dd.t for dd in data[:4]]
    # include/cssm_pf.hpp: the three routes of tests/cpp/test_hpp_forecasts.cpp print the same rows, which are this binding's
    lib = os.path.join(ROOT, "composablestatespacemodels_amd", "csrc")
    exe = str(tmp_path / "test_hpp_forecasts")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_hpp_forecasts.cpp"),
                           "-L" + lib, "-lcssm_pf", "-Wl,-rpath," + lib, "-o", exe])
    text = subprocess.run([exe, "1000"], capture_output=True, text=True, check=True).stdout.strip().splitlines()
    by = {r: [ln.split()[2:] for ln in text if ln.startswith(r + " ")] for r in ("batch", "more", "stream")}
    tt = np.arange(8.0); yy = np.array([2, 1, 4, 0, 3, 2, 5, 1.0]); hh = np.ones(8, dtype=np.uint8); hh[3] = 0
    with NativePf(model, 1000, SEED) as g:
        r = g.filter_forecasts(tt, yy, hh, None, 0.9)
    rows = [[float(tt[s]).hex(), float(r["obs_mean"][s]).hex(), float(r["eta_lower"][s]).hex(), float(r["state_upper"][s, 0]).hex()] for s in range(8)]
    for route in by:
        assert float.fromhex(by[route][0][0]) == r["ll"] and int(by[route][0][2]) == 8, route
        assert [[float.fromhex(v) for v in row] for row in by[route][1:]] == [[float.fromhex(v) for v in row] for row in rows], route


# 10 -----------------------------------------------------------------------------------------------------------------------------
def test_refusals_by_code_and_message():
    lib = _abi.load_library()
    dp = C.POINTER(C.c_double)
    t, y, has = series()
    tp, yp = t.ctypes.data_as(dp), y.ctypes.data_as(dp)
    outs = [None] * 11
    batch = (lib.cssm_pf_filter_forecasts, lib.cssm_pf_filter_forecasts_more)

    def still_filters(g, model, n, tt, yy, hh, **kw):
        """after a refusal the handle filters to the bits of a fresh one"""
        with NativePf(model, n, SEED, **kw) as f:
            assert g.run(tt, yy, hh)[0] == f.run(tt, yy, hh)[0]
            np.testing.assert_array_equal(g.particles(), f.particles())

    with NativePf(cases.c2_model(), 1000, SEED) as g:
        for fn in batch:
            assert fn(g._h, None, yp, None, 12, None, 0.975, None, None, None, *outs) == _abi.CSSM_EINVAL_ARG and b"null argument" in lib.cssm_last_error()
            assert fn(g._h, tp, None, None, 12, None, 0.975, None, None, None, *outs) == _abi.CSSM_EINVAL_ARG and b"null argument" in lib.cssm_last_error()
            assert fn(g._h, tp, yp, None, 0, None, 0.975, None, None, None, *outs) == _abi.CSSM_EINVAL_ARG and b"empty data" in lib.cssm_last_error()
            for bad in (0.0, 1.5, float("nan")):
                assert fn(g._h, tp, yp, None, 12, None, bad, None, None, None, *outs) == _abi.CSSM_EINVAL_ARG and b"interval must be in (0, 1]" in lib.cssm_last_error()
        # never initialised
        assert lib.cssm_pf_filter_forecasts_more(g._h, tp, yp, None, 12, None, 0.975, None, None, None, *outs) == _abi.CSSM_ESTATE
        assert b"continuing a filter needs an initialised handle" in lib.cssm_last_error()
        assert lib.cssm_pf_step_forecast(g._h, 0.0, 1.0, 1, 0, 0, 0.975, None, None, *outs) == _abi.CSSM_ESTATE and b"before cssm_pf_init" in lib.cssm_last_error()
        ms = np.full(2, 7.0)
        assert lib.cssm_pf_forecasts_last_ms(g._h, ms.ctypes.data_as(dp)) == _abi.CSSM_ESTATE and list(ms) == [7.0, 7.0]
        with pytest.raises(CssmError):
            g.filter_forecasts(t, y, has, interval=0.0)
        still_filters(g, cases.c2_model(), 1000, t, y, has)
        assert lib.cssm_pf_step_forecast(g._h, 20.0, 1.0, 1, 0, 0, 1.5, None, None, *outs) == _abi.CSSM_EINVAL_ARG
        # every output may be null: the call still filters, and the handle is cssm_pf_ll_filter's
        ll = C.c_double()
        assert lib.cssm_pf_filter_forecasts(g._h, tp, yp, has.ctypes.data_as(C.POINTER(C.c_uint8)), 12, None, 0.975, C.byref(ll), None, None, *outs) == 0
        with NativePf(cases.c2_model(), 1000, SEED) as f:
            assert f.run(t, y, has)[0] == ll.value
            np.testing.assert_array_equal(f.particles(), g.particles())
    # LGCP: cssm_pf_forecast's code and message
    et, ey, eh = cases.event_times(6)
    with NativePf(cases.c4_model(), 500, SEED, lgcp_precision=1) as g:
        for fn in batch:
            assert fn(g._h, et.ctypes.data_as(dp), ey.ctypes.data_as(dp), None, 6, None, 0.975, None, None, None, *outs) == _abi.CSSM_EINVAL_ARG
            assert b"LogGaussianCox" in lib.cssm_last_error()
            g.init(0.0)                                                      # (_more: a handle never initialised is refused first)
        assert lib.cssm_pf_step_forecast(g._h, 1.0, 1.0, 1, 0, 0, 0.975, None, None, *outs) == _abi.CSSM_EINVAL_ARG and b"LogGaussianCox" in lib.cssm_last_error()
        assert lib.cssm_pf_forecast(g._h, et.ctypes.data_as(dp), 1, KEY, 0.975, *([None] * 10)) == _abi.CSSM_EINVAL_ARG
        assert b"LogGaussianCox" in lib.cssm_last_error()
        still_filters(g, cases.c4_model(), 500, et, ey, eh, lgcp_precision=1)
    # a model without the scale its observation draw needs (cases.beta_model: no shape)
    bt, by_, bh = cases.unit_interval_series(6)
    with NativePf(cases.beta_model(), 500, SEED) as g:
        for fn in batch:
            assert fn(g._h, bt.ctypes.data_as(dp), by_.ctypes.data_as(dp), None, 6, None, 0.975, None, None, None, *outs) == _abi.CSSM_EINVAL_ARG
            assert b"Must provide shape parameter for Beta Model" in lib.cssm_last_error()
            g.init(0.0)
        assert lib.cssm_pf_step_forecast(g._h, 1.0, 0.5, 1, 0, 0, 0.975, None, None, *outs) == _abi.CSSM_EINVAL_ARG
        assert b"Must provide shape parameter for Beta Model" in lib.cssm_last_error()
        with pytest.raises(CssmError):
            g.filter_forecasts(bt, by_, bh)
        still_filters(g, cases.beta_model(), 500, bt, by_, bh)
    h = C.c_void_p()                                                         # the only shard of a cloud of 1000, on the default stream
    _abi.check(lib.cssm_pf_create_shard(cases.c2_model().descriptor().ptr(), 1000, 0, 1000, SEED, 0, None, C.byref(h)))
    try:
        for fn in batch:
            assert fn(h, tp, yp, None, 12, None, 0.975, None, None, None, *outs) == _abi.CSSM_ESTATE and b"sharded handle" in lib.cssm_last_error()
        assert lib.cssm_pf_step_forecast(h, 0.0, 1.0, 1, 0, 0, 0.975, None, None, *outs) == _abi.CSSM_ESTATE and b"sharded handle" in lib.cssm_last_error()
    finally:
        lib.cssm_pf_destroy(h)
    with pytest.raises(CssmError):                                           # FilterLgcp raises the refusal
        from composablestatespacemodels_amd.filter import FilterLgcp
        FilterLgcp(cases.c4_model(), Resampling.systematicResampling, 1, seed=SEED).filterForecasts([Data(float(a), 1.0) for a in et], 500)
