/*
 * cssm_obs_draws.h -- observation samplers of the numerics contract: `mod.observation(gamma).draw` of every observation model
 * (model/Model.scala:145-150, 169-180, 209-213, 242-246, 267, 282-292, 316, 340-342), as the forecasts of
 * model/ParticleFilter.scala:368-409 and model/Data.scala:196-231 draw them.
 *
 * Plain C99 over include/cssm_numerics.h, compiled unchanged by gcc (host) and by hipcc for gfx950 (device), both with
 * -ffp-contract=off: the only elementary functions are cssm_exp, cssm_log, cssm_lgamma, cssm_sqrt, cssm_fma, cssm_u01* and
 * cssm_normal_pair64, plus the exact __builtin_floor / __builtin_fabs -- no libm or OCML call, so a host build and the device
 * give the same bits.  A separate header so that the hipRTC sources and the oracle build (which include cssm_numerics.h)
 * do not change, and no existing variate does either.
 *
 * Counter layout.  Observation draws have a stream tag of their own, CSSM_STREAM_OBS = 8, and ONE stream per particle (not
 * the paired streams of the transitions): counter (key, gid = global particle id, step = horizon index h, tag 8,
 * block = b).  A draw consumes whole Philox blocks in order, b = 0, 1, 2, ...; every attempt of a rejection loop takes
 * exactly one block, so attempt j of particle i at horizon h is one fixed block.  Composite draws continue the block count
 * of their first part (NegBin: the gamma's attempts, then the Poisson's).
 *
 * Algorithms, per observation model (eta = link(gamma); every reference `observation` depends on gamma only through it):
 *   Poisson(lambda)           lambda < 10: inversion by sequential search on one uniform (block 0 words 0-1); the search
 *                             stops where the cumulative sum no longer grows (u within rounding of 1).  10 <= lambda < 2^52:
 *                             PTRS (Hoermann 1993, "The transformed rejection method for generating Poisson random
 *                             variables"), one block per attempt (U from words 0-1, V from words 2-3).  Its acceptance
 *                             test needs log pmf(k) = -lambda + k log(lambda) - lgamma(k + 1) to far better than 1:
 *                             below CSSM_OBS_PTRS_DELTA_MIN = 2^26 it is that expression as written (terms of size
 *                             lambda log(lambda) cancel: absolute error < 2^-20 there, 1.1e-6 in the octave above, 4e-2
 *                             at 1e14, 43 at 2^52 -- DESIGN.md section 2 has the measured table); from 2^26 on it is
 *                             formed from delta = k - lambda (cssm_obs_ptrs_logpmf_delta: only terms of size
 *                             delta^2 / lambda are left to cancel, error < 1e-13 up to 2^52).  Draws below 2^26 are
 *                             bit for bit those of contract v8; from 2^26 to 2^52 the attempts and their blocks are
 *                             the same and only the decisions the old error got wrong differ (contract v9).
 *                             lambda >= 2^52: floor(lambda + sqrt(lambda) z) (the normal limit; doubles are integers
 *                             there).  lambda = 0 -> 0; lambda = +inf -> +inf; NaN or lambda < 0 -> NaN.
 *   Gaussian(eta, sd)         eta + sd z, z = first normal of block 0; sd = exp(scale).
 *   Gamma(shape, scale)       Marsaglia & Tsang (2000): shape >= 1 one block per attempt (z from words 0-1 through
 *                             cssm_normal_pair64, U from words 2-3, the squeeze U < 1 - 0.0331 z^4 first); shape < 1:
 *                             Gamma(shape + 1) U^(1/shape), the boost uniform U from block 0 and the attempts from block 1.
 *                             shape <= 0 or NaN -> NaN; shape = +inf -> +inf.  A boost below e^-708 is 0 (cssm_exp), so a
 *                             value that would be below DBL_MIN comes out 0 (half of all draws at shape 1e-3).
 *   NegBin(eta, size)         Gamma(size, scale = eta / size), then Poisson of it; size = exp(scale).
 *   ZIP(eta, p)               u < p ? 0 : Poisson(eta), u from block 0, the Poisson from block 1; p = logistic(scale).
 *   Bernoulli(eta)            u < eta (eta already clamped to {0, 1} beyond |gamma| > 6 by link).
 *   Student-t(eta, v, df)     eta + v t, t = z / sqrt(chi2 / df), z = first normal of block 0, chi2 = 2 Gamma(df / 2) from
 *                             block 1 on; v = exp(scale).
 *   Beta(eta, b)              X / (X + Y), X = Gamma(eta), Y = Gamma(b) (Y's blocks follow X's); b = the stored scale as it is
 *                             (BetaModel.observation, model/Model.scala:340-342).  A non-positive shape gives NaN, and so
 *                             does 0 / 0 when both gammas underflow.
 * Rejection loops give up after CSSM_OBS_MAX_ATTEMPTS attempts (the acceptance rates are above 0.88: never reached in
 * practice) and return a deterministic value (Poisson: floor(lambda); Gamma: its mode-like d = shape - 1/3), so every draw
 * terminates in bounded time on the device.
 */
#ifndef CSSM_OBS_DRAWS_H
#define CSSM_OBS_DRAWS_H

#include "cssm_numerics.h"
#include "cssm_pf.h"

#ifdef __cplusplus
extern "C++" {
#endif

#define CSSM_STREAM_OBS 8u          /* observation draws of forecasts: counter (key, gid, horizon, 8, block) */
/* Simulations from the model (cssm_simulate, cssm_fleet_simulate: SimulateData.simPompModel) under Philox key `key`, n_paths paths:
 *   x0 of path i      CSSM_STREAM_INIT, gid i, step 0, the paired streams of draw_normals -- the initial draw of a filter of n_paths
 *                     particles whose key is `key`;
 *   time index h >= 1 the transition into it on CSSM_STREAM_STEP (paired streams; the unpaired last path of an odd count draws alone)
 *                     and its observation on CSSM_STREAM_OBS (gid i), both under step h - 1 -- horizon h - 1 of cssm_pf_forecast under
 *                     the same key;
 *   time index 0      no transition; its observation on CSSM_STREAM_OBS under step CSSM_SIM_STEP_ROW0, which no horizon can take
 *                     (a call holds fewer than 2^32 - 1 times).
 * cssm_simulate_from continues a simulation: time index j of the call moves and draws under step first_step + j. */
#define CSSM_SIM_STEP_ROW0 0xFFFFFFFFu
#define CSSM_OBS_PTRS_MIN 10.0      /* Poisson: inversion below, PTRS from here on */
#ifndef CSSM_OBS_PTRS_DELTA_MIN     /* (a test moves it to 2^52 to rebuild the sampler of contract v8) */
#define CSSM_OBS_PTRS_DELTA_MIN 0x1.0p26 /* Poisson: PTRS forms its exponent from k - lambda from here on */
#endif
#define CSSM_OBS_NORMAL_MIN 0x1.0p52 /* Poisson: the normal limit from here on */
#define CSSM_OBS_MAX_ATTEMPTS 64

/* the per-model constants of a draw (cssm_obs_params_make) */
typedef struct {
  int kind;    /* CSSM_OBS_* */
  int df;      /* Student-t degrees of freedom */
  double p0;   /* Gaussian sd, NegBin size, ZIP p, Student-t v, Beta b */
} cssm_obs_params;

/* 0, or -1: the model needs the scale parameter and has none; -2: no observation distribution (LGCP) or unknown kind;
 * -3: Student-t with df < 1. */
CSSM_HD int cssm_obs_params_make(int kind, int has_scale, double scale, int df, cssm_obs_params* out) {
  out->kind = kind; out->df = df; out->p0 = 0.0;
  switch (kind) {
    case CSSM_OBS_POISSON: case CSSM_OBS_BERNOULLI: return 0;
    case CSSM_OBS_GAUSSIAN: case CSSM_OBS_NEGBIN:
      if (!has_scale) return -1;
      out->p0 = cssm_exp(scale);
      return 0;
    case CSSM_OBS_STUDENT_T:
      if (!has_scale) return -1;
      if (df < 1) return -3;
      out->p0 = cssm_exp(scale);
      return 0;
    case CSSM_OBS_ZIP: {
      if (!has_scale) return -1;
      const double ev = cssm_exp(scale);
      out->p0 = ev / (1.0 + ev);   /* exp(v) / (1 + exp(v)), model/Model.scala:284 */
      return 0;
    }
    case CSSM_OBS_BETA:
      if (!has_scale) return -1;
      out->p0 = scale;
      return 0;
    default: return -2;
  }
}

/* The joint posterior pair particle i forecasts from (cssm_pf_forecast_posterior): Streaming.createDist's `sampleOne` of the
 * posterior sample (Resampling.scala:151-154), abs(nextInt) % M, with nextInt = word 0 of the counter (key, i, 0, CSSM_STREAM_POST, 0)
 * -- the same |int32| mod M form as the handle's sampleOne index of `filter`. */
#define CSSM_STREAM_POST 9u
CSSM_HD uint32_t cssm_posterior_pick(uint64_t key, uint64_t i, uint64_t M) {
  const int32_t r = (int32_t)cssm_philox_draw(key, i, 0u, CSSM_STREAM_POST, 0u).v[0];
  const uint32_t a = r < 0 ? (uint32_t)0 - (uint32_t)r : (uint32_t)r;
  return (uint32_t)((uint64_t)a % M);
}

/* one particle's stream of Philox blocks */
typedef struct {
  uint64_t key, gid;
  uint32_t step, block;
} cssm_obs_stream;

CSSM_HD cssm_obs_stream cssm_obs_stream_at(uint64_t key, uint64_t gid, uint32_t step) {
  cssm_obs_stream s; s.key = key; s.gid = gid; s.step = step; s.block = 0u; return s;
}
CSSM_HD cssm_u32x4 cssm_obs_next(cssm_obs_stream* s) {
  const cssm_u32x4 b = cssm_philox_draw(s->key, s->gid, s->step, CSSM_STREAM_OBS, s->block);
  s->block += 1u;
  return b;
}

/* PTRS's exponent log pmf(k) = -lambda + k log(lambda) - lgamma(k + 1), as written: every draw below CSSM_OBS_PTRS_DELTA_MIN, and the
 * far tail above it (|k - lambda| >= lambda 2^-10, where the value is below -lambda 2^-21 <= -32 and its error, at most 43, decides
 * nothing: the left side is above -120). */
CSSM_HD double cssm_obs_ptrs_logpmf_direct(double lam, double loglam, double k) {
  return (-lam + k * loglam) - cssm_lgamma(k + 1.0);
}
/* The same for lambda >= CSSM_OBS_PTRS_DELTA_MIN and |k - lambda| < lambda 2^-10, from delta = k - lambda (exact) and x = delta / lambda:
 *   -lambda + k log(lambda) - log k! = delta - k log1p(x) - log(2 pi k) / 2 - 1 / (12 k) + O(k^-3)      (Stirling; k^-3 / 360 < 1e-25)
 *   delta - k log1p(x) = -delta x - k g(x),  g(x) = log1p(x) - x = -x^2/2 + x^3/3 - ... + x^7/7         (lambda x = delta; k x^8 / 8 < 5e-10,
 *                                                                                                        < 1e-30 within 6 sd)
 * The rounding of x enters in second order only: with x' = x - r / lambda, k log1p(x) = k log1p(x') + r and k x' = delta - r + delta x'. */
CSSM_HD double cssm_obs_ptrs_logpmf_delta(double lam, double k) {
  const double delta = k - lam, x = delta / lam;
  const double g = (x * x) * (-1.0 / 2.0 + x * (1.0 / 3.0 + x * (-1.0 / 4.0 + x * (1.0 / 5.0 + x * (-1.0 / 6.0 + x * (1.0 / 7.0))))));
  return ((-(delta * x) - k * g) - 0.5 * cssm_log(6.28318530717958623200 * k)) - 1.0 / (12.0 * k);
}

/* Poisson(lambda) */
CSSM_HD double cssm_obs_poisson(double lam, cssm_obs_stream* s, const double* tab) {
  if (lam != lam || lam < 0.0) return cssm_nan();
  if (lam == 0.0) return 0.0;
  if (lam > 0x1.fffffffffffffp1023) return cssm_inf();
  if (lam < CSSM_OBS_PTRS_MIN) {        /* inversion: the first k with F(k) > u */
    const cssm_u32x4 b = cssm_obs_next(s);
    const double u = cssm_u01(b.v[0], b.v[1]);
    double p = cssm_exp(-lam), F = p, k = 0.0;
    while (u >= F) {
      k = k + 1.0;
      p = p * lam / k;
      const double Fn = F + p;
      if (Fn == F) break;               /* u within rounding of 1: the tail the sum cannot resolve */
      F = Fn;
    }
    return k;
  }
  if (lam >= CSSM_OBS_NORMAL_MIN) {
    const cssm_u32x4 b = cssm_obs_next(s);
    double z0, z1;
    cssm_normal_pair64(b.v[0], b.v[1], tab, &z0, &z1);
    const double k = __builtin_floor(lam + cssm_sqrt(lam) * z0);
    return k < 0.0 ? 0.0 : k;
  }
  /* PTRS, Hoermann (1993), with the constants of the paper */
  const double slam = cssm_sqrt(lam), loglam = cssm_log(lam);
  const double bb = 0.931 + 2.53 * slam;
  const double a = -0.059 + 0.02483 * bb;
  const double invalpha = 1.1239 + 1.1328 / (bb - 3.4);
  const double vr = 0.9277 - 3.6224 / (bb - 2.0);
  const double log_invalpha = cssm_log(invalpha);
  for (int it = 0; it < CSSM_OBS_MAX_ATTEMPTS; ++it) {
    const cssm_u32x4 b = cssm_obs_next(s);
    const double U = cssm_u01(b.v[0], b.v[1]) - 0.5;
    const double V = cssm_u01_open0(b.v[2], b.v[3]);
    const double us = 0.5 - __builtin_fabs(U);
    const double k = __builtin_floor((2.0 * a / us + bb) * U + lam + 0.43);
    if (us >= 0.07 && V <= vr) return k;
    if (k < 0.0 || (us < 0.013 && V > us)) continue;
    const double lhs = (cssm_log(V) + log_invalpha) - cssm_log(a / (us * us) + bb);
    const double rhs = (lam >= CSSM_OBS_PTRS_DELTA_MIN && __builtin_fabs(k - lam) < lam * 0x1.0p-10)
                           ? cssm_obs_ptrs_logpmf_delta(lam, k) : cssm_obs_ptrs_logpmf_direct(lam, loglam, k);
    if (lhs <= rhs) return k;
  }
  return __builtin_floor(lam);
}

/* Gamma(shape, 1) */
CSSM_HD double cssm_obs_gamma1(double shape, cssm_obs_stream* s, const double* tab) {
  if (shape != shape || shape <= 0.0) return cssm_nan();
  if (shape > 0x1.fffffffffffffp1023) return cssm_inf();
  double boost = 1.0;
  double a = shape;
  if (shape < 1.0) {                    /* Gamma(a) = Gamma(a + 1) U^(1/a) */
    const cssm_u32x4 b = cssm_obs_next(s);
    boost = cssm_exp(cssm_log(cssm_u01_open0(b.v[0], b.v[1])) / shape);
    a = shape + 1.0;
  }
  const double d = a - 1.0 / 3.0;
  const double c = 1.0 / cssm_sqrt(9.0 * d);
  for (int it = 0; it < CSSM_OBS_MAX_ATTEMPTS; ++it) {
    const cssm_u32x4 b = cssm_obs_next(s);
    double z, z1;
    cssm_normal_pair64(b.v[0], b.v[1], tab, &z, &z1);
    const double U = cssm_u01_open0(b.v[2], b.v[3]);
    double v = 1.0 + c * z;
    if (v <= 0.0) continue;
    v = (v * v) * v;
    const double z2 = z * z;
    if (U < 1.0 - 0.0331 * (z2 * z2)) return (d * v) * boost;
    if (cssm_log(U) < 0.5 * z2 + d * ((1.0 - v) + cssm_log(v))) return (d * v) * boost;
  }
  return d * boost;
}

/* One observation of model p.kind given eta = link(gamma) */
CSSM_HD double cssm_obs_draw_one(const cssm_obs_params* p, double eta, cssm_obs_stream* s, const double* tab) {
  switch (p->kind) {
    case CSSM_OBS_POISSON: return cssm_obs_poisson(eta, s, tab);
    case CSSM_OBS_GAUSSIAN: {
      const cssm_u32x4 b = cssm_obs_next(s);
      double z0, z1;
      cssm_normal_pair64(b.v[0], b.v[1], tab, &z0, &z1);
      return eta + p->p0 * z0;
    }
    case CSSM_OBS_NEGBIN: {
      const double size = p->p0;
      const double lam = cssm_obs_gamma1(size, s, tab) * (eta / size);
      return cssm_obs_poisson(lam, s, tab);
    }
    case CSSM_OBS_ZIP: {
      const cssm_u32x4 b = cssm_obs_next(s);
      const double u = cssm_u01(b.v[0], b.v[1]);
      const double k = cssm_obs_poisson(eta, s, tab);   /* drawn either way, as the reference's for-comprehension does */
      return (u < p->p0) ? 0.0 : k;
    }
    case CSSM_OBS_BERNOULLI: {
      const cssm_u32x4 b = cssm_obs_next(s);
      return (cssm_u01(b.v[0], b.v[1]) < eta) ? 1.0 : 0.0;
    }
    case CSSM_OBS_STUDENT_T: {
      const cssm_u32x4 b = cssm_obs_next(s);
      double z0, z1;
      cssm_normal_pair64(b.v[0], b.v[1], tab, &z0, &z1);
      const double df = (double)p->df;
      const double chi2 = 2.0 * cssm_obs_gamma1(0.5 * df, s, tab);
      return eta + p->p0 * (z0 / cssm_sqrt(chi2 / df));
    }
    case CSSM_OBS_BETA: {
      if (p->p0 != p->p0 || p->p0 <= 0.0) return cssm_nan();
      const double x = cssm_obs_gamma1(eta, s, tab);
      const double y = cssm_obs_gamma1(p->p0, s, tab);
      return x / (x + y);
    }
    default: return cssm_nan();
  }
}

/* ---- SimulateData.simLGCP (model/Data.scala:110-149, simSdeStream :162-176): event times of a Cox process by thinning
 * (cssm_simulate_lgcp).  Additions only: a new stream tag, no existing counter or variate moves, so the contract version stays.
 *
 * Grid.  delta = 10^-precision; t_0 = start, t_k = t_(k-1) + delta (accumulated), kept while t_k <= start + (end - start).  x_0 of path i
 * is the initial draw of a filter of n_paths particles under `key` (CSSM_STREAM_INIT, step 0, paired streams); the transition into grid
 * index k >= 1 uses dt = delta exactly and step k - 1 on CSSM_STREAM_STEP (paired streams; the unpaired last path of an odd count draws
 * alone) -- the counters of cssm_simulate.  eta_k = cssm_exp(gamma_k) is stored per grid index, ub = the exact maximum of the stored
 * values (a NaN among them makes ub NaN).
 *
 * Thinning.  Candidate c = 0, 1, ... of path i is the ONE block (key, gid = i, step = c, CSSM_STREAM_THIN, 0), unpaired:
 * U = cssm_u01_open0(words 0-1), E = -cssm_log(U) / ub; V = cssm_u01(words 2-3).  t1 = last + E (the sequential sum, last = start
 * first); the loop ends at the first candidate that is not <= end (the reference's t1 > end; a NaN ends it too: ub = 0 gives E = +inf,
 * or NaN in the one case U = 1 -- no candidate either way).  k = cssm_lgcp_index = the largest k with t_k <= t1; the candidate is an
 * event iff V <= eta_k / ub.  Accepted or not, last = t1.
 *
 * Bounded work.  Before its loop a path forms ub (end - start): not finite -> CSSM_LGCP_PATH_NONFINITE (the reference would throw on a
 * rate that is not finite); above CSSM_LGCP_MAX_EXPECTED -> CSSM_LGCP_PATH_TOO_MANY; and a loop that
 * reaches CSSM_LGCP_MAX_CANDIDATES candidates stops with CSSM_LGCP_PATH_TOO_MANY.  Such a path has zero events; the call succeeds. */
#define CSSM_STREAM_THIN 10u
#define CSSM_LGCP_MAX_EXPECTED 0x1.0p20
#define CSSM_LGCP_MAX_CANDIDATES (1u << 21)
#define CSSM_LGCP_PATH_OK 0
#define CSSM_LGCP_PATH_NONFINITE 1
#define CSSM_LGCP_PATH_TOO_MANY 2

/* the status a path enters its loop with (non-zero: it takes no candidate) */
CSSM_HD int cssm_lgcp_admit(double ub, double start, double end) {
  const double expected = ub * (end - start);
  if (!(expected - expected == 0.0)) return CSSM_LGCP_PATH_NONFINITE;
  return expected > CSSM_LGCP_MAX_EXPECTED ? CSSM_LGCP_PATH_TOO_MANY : CSSM_LGCP_PATH_OK;
}

/* candidate c of path i: the waiting time E ~ Exponential(ub) and the acceptance uniform V */
CSSM_HD void cssm_lgcp_candidate(uint64_t key, uint64_t i, uint32_t c, double ub, double* E, double* V) {
  const cssm_u32x4 b = cssm_philox_draw(key, i, c, CSSM_STREAM_THIN, 0u);
  *E = -cssm_log(cssm_u01_open0(b.v[0], b.v[1])) / ub;
  *V = cssm_u01(b.v[2], b.v[3]);
}

/* The largest k < n_grid with grid_t[k] <= t1, for start = grid_t[0] <= t1 finite: the guess floor((t1 - start) / delta), corrected
 * against the accumulated grid times (they drift from start + k delta, about 1.7e-13 over 1000 steps: the guess alone is wrong at
 * cell edges). */
CSSM_HD uint32_t cssm_lgcp_index(const double* grid_t, uint32_t n_grid, double start, double delta, double t1) {
  const double q = __builtin_floor((t1 - start) / delta), top = (double)(n_grid - 1u);
  uint32_t k = q >= top ? n_grid - 1u : (q > 0.0 ? (uint32_t)q : 0u);
  while (k + 1u < n_grid && grid_t[k + 1u] <= t1) k += 1u;
  while (k > 0u && grid_t[k] > t1) k -= 1u;
  return k;
}

#ifdef __cplusplus
}
#endif
#endif /* CSSM_OBS_DRAWS_H */
