"""The law of every observation sampler of include/cssm_obs_draws.h over its documented range, on the host twin (tests/cpp/obs_draw_twin.c,
built by test_forecast_draws.build_twin the way the numerics contract prescribes).  No GPU: the device is held to the twin bit for bit
(tests/test_gpu_forecast*.py, test_gpu_simulate*.py and, where the lanes of a wavefront sit in different regimes,
tests/test_gpu_obs_draw_regimes.py), so the law of the twin is the law of the device.

Every case draws at one fixed key and is never retried: it passes or fails deterministically.  The arguments are the tables below, one
row per regime and per regime edge.  Criteria:

* discrete laws with a mean below 1e6: Pearson chi-square (cells merged to >= 5 expected), p > 1e-4;
* continuous laws: Kolmogorov-Smirnov, p > 1e-4.  Censoring is part of the law: Gamma's share of exact zeros against the law's mass
  below DBL_MIN and Beta(1e-3, 1e-3)'s share of NaN against the probability that both of its gammas underflow (from the gamma law), each
  within 4.5 binomial standard errors; a NaN anywhere else fails;
* counts with a mean >= 1e6 on z = (x - mean) / sd: mean, variance, skewness and excess kurtosis of z against the law's own (Poisson:
  0, 1, lambda^-1/2, lambda^-1; NegBin from its cumulants), each within 4.5 standard errors, the standard error of each statistic
  from the law's moments up to the eighth at N (the delta-method variances of Kendall & Stuart, vol. 1, ch. 10); Poisson from 1e8 on
  also KS of z against the normal law at the midpoint of each count's cell; max|z| <= 6 (Poisson: the law expects 8e-4 draws
  beyond it at N = 4e5).  The NegBin rows have skewness 2 / sqrt(size) and cannot be held to 6: theirs is the bound the law itself
  exceeds with the same expected count, 8e-4.

Power.  The sampler of the parent commit (PTRS's exponent formed as -lambda + k log(lambda) - lgamma(k + 1) up to 2^52) is built too and
MUST be rejected by the variance criterion at lambda = 1e15, 4e15 and the last double below 2^52; the table of both builds is printed.
Measured: the parent's variance of z is off by 16.5, 231 and 42 standard errors there (its kurtosis by 57, 306 and 138), the fixed
sampler's by at most 1.7 on every row, and no statistic of it by more than 1.7.
"""
from __future__ import annotations

import ctypes as C
import json
import math
import os
import subprocess

import numpy as np
import pytest

from test_forecast_draws import (BERNOULLI, BETA, GAUSSIAN, KEY, NEGBIN, POISSON, ROOT, STUDENT_T, ZIP, _dp, build_twin, chi2_pvalue,
                                 draws)

stats = pytest.importorskip("scipy.stats")
mp = pytest.importorskip("mpmath")

N = 400_000
SE = 4.5
DBL_MAX, DBL_MIN = float.fromhex("0x1.fffffffffffffp1023"), float.fromhex("0x1.0p-1022")
CUT = 2.0 ** 26           # CSSM_OBS_PTRS_DELTA_MIN
below = lambda x: float(np.nextafter(x, 0.0))

POISSON_SMALL = [1e-300, 1e-3, 3.0, below(10.0), 10.0, 30.0, 1e4]                              # chi-square
POISSON_LARGE = [1e8, below(CUT), CUT, 1e12, 1e14, 1e15, 4e15, below(2.0 ** 52), 2.0 ** 52, 1e18]   # moments of z
POISSON_EXACT = [(0.0, 0.0), (math.inf, math.inf), (math.nan, math.nan), (-1.0, math.nan)]
GAMMA_SHAPES = [1e-3, 1e-2, 0.5, below(1.0), 1.0, 3.0, 1e2, 1e6, 1e12]
GAMMA_EXACT = [(0.0, math.nan), (-1.0, math.nan), (math.nan, math.nan), (math.inf, math.inf)]
NEGBIN_SMALL = [(0.05, 2.0), (3.0, 4.0), (1e6, 5.0)]
NEGBIN_LARGE = [(3.0, 1e6), (0.5, 1e10), (2.0, 1e15)]
ZIP_ROWS = [(p, lam) for p in (0.01, 0.5, 0.99) for lam in (0.5, 50.0)]
T_DF = [1, 2, 30, 1000, 10 ** 6]
BETA_ROWS = [(0.3, 2.0), (4.0, 0.5), (1e-2, 5.0), (1e3, 1e3), (1e6, 2.0), (0.5, 1e6)]
BERNOULLI_ETA = [0.0, 1e-6, 0.5, 1.0]
GAUSSIAN_SD = [1e-8, 1.0, 1e8]
PARENT_REJECTED = [1e15, 4e15, below(2.0 ** 52)]


# ---------------------------------------------------------------- the two builds

def _bind_exponents(lib):
    for f in (lib.twin_ptrs_logpmf_direct, lib.twin_ptrs_logpmf_delta):
        f.argtypes = [C.c_double, C.c_double]
        f.restype = C.c_double
    return lib


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    return _bind_exponents(build_twin(tmp_path_factory.mktemp("twin")))


def _parent_header_from_git():
    """The newest committed include/cssm_obs_draws.h that forms PTRS's exponent directly everywhere (the parent commit's: HEAD~ once this
    change is committed), or None where the checkout has no history."""
    try:
        revs = subprocess.run(["git", "log", "--format=%H", "--", "include/cssm_obs_draws.h"], cwd=ROOT, capture_output=True, text=True,
                              timeout=60)
        for rev in revs.stdout.split():
            blob = subprocess.run(["git", "show", rev + ":include/cssm_obs_draws.h"], cwd=ROOT, capture_output=True, text=True, timeout=60)
            if blob.returncode == 0 and blob.stdout and "CSSM_OBS_PTRS_DELTA_MIN" not in blob.stdout:
                return blob.stdout
    except (OSError, subprocess.SubprocessError):
        pass
    return None


def _build_parent(out_dir, header_text):
    """The twin over the parent's header (header_text), or -- header_text None -- over today's header with the cut moved to 2^52, where
    the normal limit takes over: the parent's arithmetic statement for statement."""
    inc = os.path.join(str(out_dir), "include")
    cpp = os.path.join(str(out_dir), "tests", "cpp")
    os.makedirs(inc); os.makedirs(cpp)
    for name in ("cssm_numerics.h", "cssm_pf.h", "cssm_obs_draws.h"):
        with open(os.path.join(ROOT, "include", name)) as src, open(os.path.join(inc, name), "w") as dst:
            dst.write(header_text if (name == "cssm_obs_draws.h" and header_text is not None) else src.read())
    with open(os.path.join(ROOT, "tests", "cpp", "obs_draw_twin.c")) as src, open(os.path.join(cpp, "obs_draw_twin.c"), "w") as dst:
        text = src.read()
        dst.write(text if header_text is None else text[:text.index("/* PTRS's exponent")])   # the parent has no such functions
    so = os.path.join(str(out_dir), "parent_twin.so")
    flags = ["-DCSSM_OBS_PTRS_DELTA_MIN=0x1.0p52"] if header_text is None else []
    subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-mfma", "-std=c99", "-shared", "-fPIC", *flags, "-o", so,
                           os.path.join(cpp, "obs_draw_twin.c"), "-lm"])
    lib = C.CDLL(so)
    lib.twin_obs_draw.argtypes = [C.c_int, _dp, C.c_size_t, C.c_int, C.c_double, C.c_int, C.c_uint64, C.c_uint32, _dp]
    lib.twin_obs_draw_at.argtypes = [C.c_int, C.c_double, C.c_int, C.c_double, C.c_int, C.c_uint64, C.c_uint64, C.c_uint32,
                                     C.POINTER(C.c_uint32)]
    lib.twin_obs_draw_at.restype = C.c_double
    return lib


@pytest.fixture(scope="module")
def parent(tmp_path_factory):
    """(from git or None, from today's header with the cut at 2^52)"""
    text = _parent_header_from_git()
    return (_build_parent(tmp_path_factory.mktemp("parent_git"), text) if text is not None else None,
            _build_parent(tmp_path_factory.mktemp("parent_knob"), None))


# ---------------------------------------------------------------- moments of the law

def _central_from_cumulants(k):
    """Standardised central moments mu_3 .. mu_8 (mu_2 = 1) from the cumulants k[1..8]."""
    s = math.sqrt(k[2])
    c = [0.0, 0.0, 1.0] + [k[n] / s ** n for n in range(3, 9)]
    mu = [1.0, 0.0, 1.0, c[3], c[4] + 3.0, c[5] + 10.0 * c[3], c[6] + 15.0 * c[4] + 10.0 * c[3] ** 2 + 15.0,
          c[7] + 21.0 * c[5] + 35.0 * c[4] * c[3] + 105.0 * c[3],
          c[8] + 28.0 * c[6] + 56.0 * c[5] * c[3] + 35.0 * c[4] ** 2 + 210.0 * c[4] + 280.0 * c[3] ** 2 + 105.0]
    return mu


def _stirling2(n, j):
    return sum((-1) ** (j - i) * math.comb(j, i) * i ** n for i in range(j + 1)) // math.factorial(j)


def poisson_cumulants(lam):
    return [0.0] + [lam] * 8


def negbin_cumulants(size, mu):
    """K(t) = -size log(1 - q (e^t - 1)), q = mu / size: kappa_n = size sum_j (j - 1)! S(n, j) q^j."""
    q = mu / size
    return [0.0] + [size * sum(math.factorial(j - 1) * _stirling2(n, j) * q ** j for j in range(1, n + 1)) for n in range(1, 9)]


def z_statistics(z):
    m = z.mean()
    d = z - m
    m2 = np.mean(d * d)
    return m, m2, np.mean(d ** 3) / m2 ** 1.5, np.mean(d ** 4) / m2 ** 2 - 3.0


def z_standard_errors(mu, n):
    """Of the mean, variance, skewness and kurtosis of n standardised draws of a law with standardised central moments mu[0..8]."""
    m3, m4, m5, m6, m8 = mu[3], mu[4], mu[5], mu[6], mu[8]
    v_skew = m6 - 6.0 * m4 + 9.0 + m3 * m3 * (9.0 * m4 + 35.0) / 4.0 - 3.0 * m3 * m5
    v_kurt = m8 - 4.0 * m4 * m6 + 4.0 * m4 ** 3 - m4 * m4 + 16.0 * m4 * m3 * m3 - 8.0 * m3 * m5 + 16.0 * m3 * m3
    return tuple(math.sqrt(v / n) for v in (1.0, m4 - 1.0, v_skew, v_kurt))


def test_the_standard_errors_are_those_of_the_normal_law_in_the_limit():
    se = z_standard_errors(_central_from_cumulants(poisson_cumulants(1e30)), 1)
    assert np.allclose(se, [1.0, math.sqrt(2.0), math.sqrt(6.0), math.sqrt(24.0)], rtol=1e-12)
    # NegBin(size, mu) with size -> inf is Poisson(mu)
    assert np.allclose(negbin_cumulants(1e12, 7.0)[1:], poisson_cumulants(7.0)[1:], rtol=1e-9)
    # and its first cumulants in closed form
    k = negbin_cumulants(3.0, 4.0)
    assert np.allclose(k[1:4], [4.0, 4.0 + 16.0 / 3.0, stats.nbinom(3.0, 3.0 / 7.0).stats("s") * (4.0 + 16.0 / 3.0) ** 1.5], rtol=1e-12)


def moment_report(label, x, mean, sd, cumulants, n):
    """(row of the table, the four deviations in standard errors, max|z|, z)"""
    z = (x - mean) / sd
    got = z_statistics(z)
    mu = _central_from_cumulants(cumulants)
    want = (0.0, 1.0, mu[3], mu[4] - 3.0)
    dev = [(g - w) / s for g, w, s in zip(got, want, z_standard_errors(mu, n))]
    zmax = float(np.max(np.abs(z)))
    row = "%-26s mean %+8.5f (%+5.1f se)  var %8.5f (%+6.1f se)  skew %+8.5f (%+5.1f se)  kurt %+8.5f (%+5.1f se)  max|z| %5.2f" % (
        label, got[0], dev[0], got[1], dev[1], got[2], dev[2], got[3], dev[3], zmax)
    return row, dev, zmax, z


# ---------------------------------------------------------------- Poisson

def test_poisson_early_returns_are_exact(twin):
    for lam, want in POISSON_EXACT:
        x = draws(twin, POISSON, lam, n=256)
        assert np.array_equal(x, np.full(256, want), equal_nan=True), lam
    # at the largest finite rate sqrt(lambda) = 2^512 is far below half an ulp of lambda, 2^970: the only double within any number of
    # standard deviations is lambda itself
    assert np.all(draws(twin, POISSON, DBL_MAX, n=N) == DBL_MAX)


@pytest.mark.parametrize("lam", POISSON_SMALL)
def test_poisson_small_rates(twin, lam):
    x = draws(twin, POISSON, lam, n=N)
    assert np.all(x == np.floor(x)) and np.all(x >= 0)
    if N * -math.expm1(-lam) < 1e-6:           # the law puts less than 1e-6 expected draws off zero
        assert np.all(x == 0.0)
        return
    p = chi2_pvalue(x, stats.poisson(lam).pmf, int(lam + 8 * math.sqrt(lam) + 8))
    print("Poisson(%r): chi-square p = %.4f" % (lam, p))
    assert p > 1e-4


def _poisson_row(lib, lam, n=N):
    x = draws(lib, POISSON, lam, n=n)
    assert np.all(x == np.floor(x)) and np.all(x >= 0)
    return moment_report("Poisson(%.17g)" % lam, x, lam, math.sqrt(lam), poisson_cumulants(lam), n)


@pytest.mark.parametrize("lam", POISSON_LARGE)
def test_poisson_large_rates(twin, lam):
    row, dev, zmax, z = _poisson_row(twin, lam)
    print(row)
    assert all(abs(d) <= SE for d in dev), row
    assert zmax <= 6.0, row
    if lam >= 1e8:      # the midpoint of the count's cell under the normal law; the law's own skewness lambda^-1/2 <= 1e-4 moves the cdf by < 1e-5
        p = stats.kstest(z, stats.norm.cdf).pvalue
        print("  KS against the normal law: p = %.4f" % p)
        assert p > 1e-4


def test_the_parent_commits_sampler_is_rejected(twin, parent):
    """The table of both builds, and the power of the criteria above: the parent's header fails them where its exponent is noise."""
    from_git, from_knob = parent
    if from_git is not None:      # the two ways to the parent's sampler are one sampler
        for lam in (30.0, 1e6, below(CUT), CUT, 1e12, 1e15, below(2.0 ** 52)):
            a, b = draws(from_git, POISSON, lam, n=20_000), draws(from_knob, POISSON, lam, n=20_000)
            assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), lam
    old = from_git if from_git is not None else from_knob
    print("\nparent commit (from %s)" % ("git" if from_git is not None else "the cut moved to 2^52"))
    rejected = {}
    for lam in POISSON_LARGE:
        row, dev, zmax, _ = _poisson_row(old, lam)
        rejected[lam] = (dev, zmax)
        print(row)
    print("this commit")
    for lam in POISSON_LARGE:
        print(_poisson_row(twin, lam)[0])
    for lam in PARENT_REJECTED:
        dev, zmax = rejected[lam]
        assert abs(dev[1]) > SE and abs(dev[3]) > SE, (lam, dev)      # variance and kurtosis both
    assert abs(rejected[1e15][0][1]) > 15 and abs(rejected[4e15][0][1]) > 200 and rejected[4e15][1] > 6.0
    # below the cut the two builds are one sampler
    for lam in (0.5, 12.0, 1e4, 1e6, below(CUT)):
        a, b = draws(old, POISSON, lam, n=50_000), draws(twin, POISSON, lam, n=50_000)
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), lam


def test_draws_below_the_cut_are_those_of_the_parent_commit(twin):
    """tests/golden/obs_draws_pins.json: the first 64 Poisson draws (particles 0..63, step 0, the test key) of the parent commit's twin and
    the blocks each consumed."""
    with open(os.path.join(ROOT, "tests", "golden", "obs_draws_pins.json")) as f:
        pins = json.load(f)
    assert int(pins["key"], 16) == KEY and float.fromhex(pins["cut"]) == CUT
    assert [float.fromhex(r["lambda"]) for r in pins["poisson"]] == [0.5, 12.0, 1e4, 1e6, below(CUT)]
    for r in pins["poisson"]:
        lam = float.fromhex(r["lambda"])
        assert len(r["draws"]) == 64 and len(r["blocks"]) == 64
        for gid, (want, blocks) in enumerate(zip(r["draws"], r["blocks"])):
            b = C.c_uint32()
            got = twin.twin_obs_draw_at(POISSON, lam, 0, 0.0, 0, KEY, gid, 0, C.byref(b))
            assert got.hex() == want and b.value == blocks, (lam, gid)


# ---------------------------------------------------------------- PTRS's exponent against 60-digit arithmetic

def _logpmf_ref(lam, k):
    lam, k = mp.mpf(lam), mp.mpf(k)
    return -lam + k * mp.log(lam) - mp.loggamma(k + 1)


def _exponent_error(fn, e, fractions=(0.0, 0.173, 0.3717, 0.5, 0.91, 1.0)):
    """max |fn - exact| over lambda in the octave [2^e, 2^(e+1)) and k = lambda + {-4 .. 4} sqrt(lambda) in eighths"""
    worst = 0.0
    for fr in fractions:
        lam = below(2.0 ** (e + 1)) if fr == 1.0 else 2.0 ** e * (1.0 + fr)
        for j in range(-32, 33):
            k = math.floor(lam + j / 8.0 * math.sqrt(lam))
            worst = max(worst, abs(float(mp.mpf(fn(lam, float(k))) - _logpmf_ref(lam, k))))
    return worst


def test_ptrs_exponent_error_is_below_2_to_minus_20_where_each_form_serves(twin):
    """log V has a density <= 1, so an error eps of the exponent flips at most a share eps of the acceptance decisions: 2^-20 is three
    orders below what 4e5 draws resolve.  The direct form keeps it up to 2^26 and loses it in the octave above (which is what set the
    cut: DESIGN.md section 2 has the table); the form in k - lambda keeps it, with eight orders to spare, up to 2^52."""
    with mp.workdps(60):
        print("\noctave   direct form   form in k - lambda")
        for e in range(20, 52):
            direct, delta = _exponent_error(twin.twin_ptrs_logpmf_direct, e), _exponent_error(twin.twin_ptrs_logpmf_delta, e)
            print("2^%-2d   %12.3e   %12.3e" % (e, direct, delta))
            if 2.0 ** e < CUT:
                assert direct < 2.0 ** -20, e
            else:
                assert delta < 2.0 ** -20, e
            if e >= 27:
                assert direct > 2.0 ** -20, e     # why the cut cannot sit higher
        # the far tail handed to the direct form (|k - lambda| >= lambda 2^-10): the value is below -32, the left side above -120
        for lam in (CUT, 1e12, below(2.0 ** 52)):
            for sgn in (-1.0, 1.0):
                k = math.floor(lam + sgn * lam * 2.0 ** -10)
                assert float(_logpmf_ref(lam, k)) < -32.0 + 1e-3
                assert abs(twin.twin_ptrs_logpmf_delta(lam, float(k)) - float(_logpmf_ref(lam, k))) < 2.0 ** -20 * max(1.0, lam * 2.0 ** -21)


# ---------------------------------------------------------------- Gamma

def _gamma(twin, shape, n):
    out = np.zeros(n)
    twin.twin_gamma(shape, n, KEY, 3, out.ctypes.data_as(_dp))
    return out


def test_gamma_early_returns_are_exact(twin):
    for shape, want in GAMMA_EXACT:
        assert np.array_equal(_gamma(twin, shape, 256), np.full(256, want), equal_nan=True), shape


@pytest.mark.parametrize("shape", GAMMA_SHAPES)
def test_gamma_over_its_range(twin, shape):
    x = _gamma(twin, shape, N)
    assert not np.any(np.isnan(x)) and np.all(x >= 0)
    law = stats.gamma(shape)
    q = float(law.cdf(DBL_MIN))                  # the mass the sampler flushes to zero
    share = float(np.mean(x == 0.0))
    margin = SE * math.sqrt(q * (1.0 - q) / N)
    print("Gamma(%r): zeros %.5f, law below DBL_MIN %.5f +- %.5f" % (shape, share, q, margin))
    assert abs(share - q) <= margin
    # the flush acts on the boost U^(1/shape), not on the product: a few draws (2e-4 at shape 1e-3) come out subnormal instead of zero.
    # They are below DBL_MIN all the same: censored, for the sample as for the law
    assert abs(float(np.mean(x < DBL_MIN)) - q) <= margin
    rest = x[x >= DBL_MIN]
    p = stats.kstest(rest, lambda t: (law.cdf(t) - q) / (1.0 - q)).pvalue
    print("  KS of the rest: p = %.4f" % p)
    assert p > 1e-4


# ---------------------------------------------------------------- NegBin, ZIP, Bernoulli

@pytest.mark.parametrize("size,mu", NEGBIN_SMALL)
def test_negative_binomial_small_means(twin, size, mu):
    x = draws(twin, NEGBIN, mu, n=N, has_scale=1, scale=math.log(size))
    assert np.all(x == np.floor(x)) and np.all(x >= 0)
    law = stats.nbinom(size, size / (size + mu))
    p = chi2_pvalue(x, law.pmf, int(law.isf(1e-9)) + 2)
    print("NegBin(size %r, mean %r): chi-square p = %.4f" % (size, mu, p))
    assert p > 1e-4


@pytest.mark.parametrize("size,mu", NEGBIN_LARGE)
def test_negative_binomial_large_means(twin, size, mu):
    x = draws(twin, NEGBIN, mu, n=N, has_scale=1, scale=math.log(size))
    assert np.all(x == np.floor(x)) and np.all(x >= 0)
    sd = math.sqrt(mu + mu * mu / size)
    row, dev, zmax, z = moment_report("NegBin(%g, %g)" % (size, mu), x, mu, sd, negbin_cumulants(size, mu), N)
    # the bound the law exceeds with 8e-4 expected draws (4e-4 per side): the gamma mixing law's quantile and six Poisson sd around it
    g = stats.gamma(size, scale=mu / size)
    hi, lo = float(g.isf(4e-4 / N)), float(g.ppf(4e-4 / N))
    bound = max((hi + 6.0 * math.sqrt(hi) - mu) / sd, (mu - max(0.0, lo - 6.0 * math.sqrt(lo))) / sd)
    print(row + "  (law's bound %.2f)" % bound)
    assert all(abs(d) <= SE for d in dev), row
    assert zmax <= bound, row


@pytest.mark.parametrize("p0,lam", ZIP_ROWS)
def test_zero_inflated_poisson_rows(twin, p0, lam):
    x = draws(twin, ZIP, lam, n=N, has_scale=1, scale=math.log(p0 / (1.0 - p0)))
    assert np.all(x == np.floor(x)) and np.all(x >= 0)
    pmf = lambda k: (1.0 - p0) * stats.poisson(lam).pmf(k) + p0 * (k == 0)
    p = chi2_pvalue(x, pmf, int(lam + 8 * math.sqrt(lam) + 8))
    print("ZIP(p %r, rate %r): chi-square p = %.4f" % (p0, lam, p))
    assert p > 1e-4


@pytest.mark.parametrize("eta", BERNOULLI_ETA)
def test_bernoulli_rows(twin, eta):
    x = draws(twin, BERNOULLI, eta, n=N)
    assert np.all((x == 0.0) | (x == 1.0))
    if eta in (0.0, 1.0):
        assert np.all(x == eta)
        return
    ones = int(x.sum())
    print("Bernoulli(%r): %d ones of %d" % (eta, ones, N))
    assert stats.binomtest(ones, N, eta).pvalue > 1e-4


# ---------------------------------------------------------------- Gaussian, Student-t, Beta

@pytest.mark.parametrize("sd", GAUSSIAN_SD)
def test_gaussian_rows(twin, sd):
    eta = -1.25
    x = draws(twin, GAUSSIAN, eta, n=N, has_scale=1, scale=math.log(sd))
    assert not np.any(np.isnan(x))
    # (eta + sd z rounds at 2e-16, which is 2e-8 of sd at sd = 1e-8: far below what the test resolves)
    p = stats.kstest((x - eta) / sd, stats.norm.cdf).pvalue
    print("Gaussian(sd %r): KS p = %.4f" % (sd, p))
    assert p > 1e-4


@pytest.mark.parametrize("df", T_DF)
def test_students_t_rows(twin, df):
    v, eta = 0.6, 0.5
    x = draws(twin, STUDENT_T, eta, n=N, has_scale=1, scale=math.log(v), df=df)
    assert not np.any(np.isnan(x))
    p = stats.kstest((x - eta) / v, stats.t(df).cdf).pvalue
    print("Student-t(df %d): KS p = %.4f" % (df, p))
    assert p > 1e-4


@pytest.mark.parametrize("a,b", BETA_ROWS)
def test_beta_rows(twin, a, b):
    x = draws(twin, BETA, a, n=N, has_scale=1, scale=b)
    assert not np.any(np.isnan(x)) and np.all((x >= 0) & (x <= 1))
    p = stats.kstest(x, stats.beta(a, b).cdf).pvalue
    print("Beta(%r, %r): KS p = %.4f" % (a, b, p))
    assert p > 1e-4


def test_beta_where_both_gammas_underflow(twin):
    """Beta(1e-3, 1e-3): X / (X + Y) is NaN where both gammas are flushed to zero, with probability P(Gamma(1e-3) < DBL_MIN)^2 = 0.2425
    from the gamma law.  Of the rest, which sits at 0 and 1 to within rounding for all but a small share, the law's cdf
    P(X / (X + Y) <= t, not both flushed) / (1 - q^2) is held at cut points between the atoms (a quadrature over Y's cdf)."""
    a = 1e-3
    x = draws(twin, BETA, a, n=N, has_scale=1, scale=a)
    law = stats.gamma(a)
    q = float(law.cdf(DBL_MIN))
    nan_share, want = float(np.mean(np.isnan(x))), q * q
    margin = SE * math.sqrt(want * (1.0 - want) / N)
    print("Beta(1e-3, 1e-3): NaN share %.5f, law %.5f +- %.5f" % (nan_share, want, margin))
    assert abs(nan_share - want) <= margin
    rest = x[~np.isnan(x)]
    assert np.all((rest >= 0) & (rest <= 1))
    v = q + (1.0 - q) * (np.arange(200_000) + 0.5) / 200_000          # Y's cdf over Y >= DBL_MIN, midpoints
    y = law.ppf(v)
    for t in (1e-300, 1e-100, 1e-10, 0.5, 1.0 - 1e-10):
        with np.errstate(over="ignore", under="ignore"):
            both = np.mean(np.maximum(law.cdf(y * (t / (1.0 - t))) - q, 0.0)) * (1.0 - q)     # X and Y >= DBL_MIN, X / (X + Y) <= t
        cdf = (q * (1.0 - q) + both) / (1.0 - q * q)                                          # X flushed, Y not: exactly 0
        got = float(np.mean(rest <= t))
        m = SE * math.sqrt(cdf * (1.0 - cdf) / rest.size)
        print("  P(B <= %g | not NaN): %.5f, law %.5f +- %.5f" % (t, got, cdf, m))
        assert abs(got - cdf) <= m
