/* if2_twin.c -- a sequential statement of the contract's iterated filtering (include/cssm_numerics.h, "iterated filtering"; EXTENSION),
 * written from that header alone (gcc -O2 -ffp-contract=off -mfma), loaded with ctypes by tests/test_fleet_if2_host.py and
 * tests/test_gpu_fleet_if2.py: ONE search of cssm_fleet_if2, particle after particle.
 *
 * layout   cssm_fleet_if2_layout's integers: d, n_theta, obs_kind, obs_df, scale slot; per component sde_kind, leaf, index in the leaf,
 *          f_kind, period and the slots of m0, c0, mu, phi, sigma; then n_theta ivp flags
 * swarm    [n_theta][n]   in: the starting swarm; out: the swarm behind the last iteration that completed
 * cool     [n_iters]      cssm_fleet_if2_cooling's array (the host's pow, handed to the device and to this program alike)
 * t, y, has [T]           the series; the first increment starts at the smallest time
 * mean [n_iters][n_theta], ll [n_iters]: rows of the iterations that completed (the others are left alone)
 * ll_t, ess_t [T], x_out [d][n], anc_out [n]: of the last iteration, may be NULL
 * returns 0, or -5 (CSSM_ENONFINITE) with *fail_iter = the iteration in which no particle of some record had a usable weight */
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/cssm_numerics.h"

/* normal number q of the filter's stream of particle i (particles 2m and 2m + 1 share stream m; particle i owns q = (i & 1) d + k) */
static double filter_normal(uint64_t key, uint32_t i, uint32_t step, uint32_t tag, int d, int k) {
  const uint32_t q = (i & 1u) * (uint32_t)d + (uint32_t)k;
  double z0, z1;
  cssm_normal_pair_of(key, (uint64_t)(i >> 1), step, tag, q >> 1, CSSM_LOG_TAB, &z0, &z1);
  return (q & 1u) ? z1 : z0;
}

/* the transition coefficients of a component over dt (the filter's coefficient function) */
static void sde_coef(int kind, double mu, double phi, double sigma, double dt, double* p) {
  p[0] = 0.0; p[1] = 0.0; p[2] = 0.0; p[3] = 0.0;
  if (kind == 0) { p[3] = cssm_sqrt(sigma * dt); }
  else if (kind == 1) { p[0] = mu * dt; p[3] = cssm_sqrt(sigma * dt); }
  else if (kind == 2) {
    const double var = (sigma * sigma / (phi * 2.0)) * (1.0 - cssm_exp(phi * -2.0 * dt));
    p[0] = mu; p[1] = cssm_exp(-phi * dt); p[3] = cssm_sqrt(var);
  } else { p[0] = mu; p[1] = phi; p[2] = sigma; p[3] = cssm_sqrt(dt); }
}
/* ... and the transition on them (the filter's statement) */
static double transition(int kind, const double* p, double dt, double x, double z) {
  if (kind == 0) return p[3] * z + x;
  if (kind == 1) { const double mean = x + p[0]; return p[3] * z + mean; }
  if (kind == 2) { const double mean = p[0] + (x - p[0]) * p[1]; return p[3] * z + mean; }
  { const double dW = p[3] * z, a = (p[0] + p[1] * x) * dt, b = p[2] * dW; return (x + a) + b; }
}

typedef struct { int kind, leaf, idx, f_kind, period, slot[5]; } comp_t;

static double field(const comp_t* c, int f, const double* th, uint32_t n, uint32_t i) {
  return c->slot[f] < 0 ? 0.0 : cssm_constrain(c->kind, f, th[(size_t)c->slot[f] * n + i]);
}

int twin_if2(const int32_t* layout, uint32_t n, double* swarm, const double* rw_sd, const double* cool, uint32_t first_iter, uint32_t n_iters,
             uint64_t seed, uint32_t T, const double* t, const double* y, const uint8_t* has, double* mean, double* ll_out, double* ll_t,
             int32_t* ess_t, double* x_out, uint32_t* anc_out, uint32_t* fail_iter) {
  const int d = layout[0], nt = layout[1], obs = layout[2];
  const double df = (double)layout[3];
  const int scale_slot = layout[4];
  const int32_t* ivp = layout + 5 + 10 * d;
  comp_t comp[16];
  for (int k = 0; k < d; ++k) {
    const int32_t* o = layout + 5 + 10 * k;
    comp[k].kind = o[0]; comp[k].leaf = o[1]; comp[k].idx = o[2]; comp[k].f_kind = o[3]; comp[k].period = o[4];
    for (int f = 0; f < 5; ++f) comp[k].slot[f] = o[5 + f];
  }
  const int scaled = obs == 1 || obs == 3 || obs == 4 || obs == 6, own_level = obs == 1 || obs == 6;
  double* th[2] = {(double*)malloc((size_t)nt * n * 8u), (double*)malloc((size_t)nt * n * 8u)};
  double* x[2] = {(double*)malloc((size_t)d * n * 8u), (double*)malloc((size_t)d * n * 8u)};
  double* w = (double*)malloc((size_t)n * 8u);
  double* tree = (double*)malloc((size_t)n * 8u);
  uint32_t* anc = (uint32_t*)malloc((size_t)n * 4u);
  int rc = 0;
  if (!th[0] || !th[1] || !x[0] || !x[1] || !w || !tree || !anc) { rc = -1; goto done; }
  double t0 = t[0];
  for (uint32_t s = 1; s < T; ++s) t0 = (t[s] < t0) ? t[s] : t0;
  for (uint32_t q = 0; q < n_iters && !rc; ++q) {
    const uint32_t m = first_iter + q;
    const uint64_t key = cssm_derive_key(seed, (uint64_t)m + 1u);
    /* the swarm perturbed (every slot), x0 from the particle's own m0 and c0, identity ancestors */
    for (uint32_t i = 0; i < n; ++i) {
      for (int j = 0; j < nt; ++j) {
        const double sdc = rw_sd[j] * cool[q];
        double v = swarm[(size_t)j * n + i];
        if (sdc != 0.0) v = cssm_if2_perturb(v, sdc, cssm_if2_normal(key, i, 0u, (uint32_t)j, CSSM_LOG_TAB));
        th[0][(size_t)j * n + i] = v;
      }
      for (int k = 0; k < d; ++k)
        x[0][(size_t)k * n + i] = cssm_sqrt(field(&comp[k], 1, th[0], n, i)) * filter_normal(key, i, 0u, CSSM_STREAM_INIT, d, k) + field(&comp[k], 0, th[0], n, i);
      anc[i] = i;
    }
    double ll = 0.0, tp = t0;
    int32_t ess = (int32_t)n;
    for (uint32_t r = 0; r < T && !rc; ++r) {
      const double dt = t[r] - tp;
      const int weighted = has ? has[r] != 0 : 1;
      const double* ts = th[r & 1u]; double* td = th[(r & 1u) ^ 1u];
      const double* xs = x[r & 1u]; double* xd = x[(r & 1u) ^ 1u];
      const double ypart = cssm_obs_ypart(obs, y[r], df), yk = cssm_obs_y(obs, y[r]);
      double fco[16];
      for (int k = 0; k < d; ++k) {                             /* F(t_r): the first component of a leaf, or the seasonal harmonics */
        if (comp[k].f_kind == 0) fco[k] = comp[k].idx == 0 ? 1.0 : 0.0;
        else {
          double sn, cs;
          cssm_sincos2pi(cssm_seasonal_phase((double)(comp[k].idx / 2 + 1), t[r], (double)comp[k].period), &sn, &cs);
          fco[k] = (comp[k].idx & 1) ? sn : cs;
        }
      }
      uint64_t kmax = cssm_order_key(-cssm_inf()), kcmax = kmax;   /* the maxima under the order of cssm_order_key */
      for (uint32_t i = 0; i < n; ++i) {
        const uint32_t a = anc[i];
        for (int j = 0; j < nt; ++j) {
          const double sdc = ivp[j] ? 0.0 : rw_sd[j] * cool[q];
          double v = ts[(size_t)j * n + a];
          if (sdc != 0.0) v = cssm_if2_perturb(v, sdc, cssm_if2_normal(key, i, r + 1u, (uint32_t)j, CSSM_LOG_TAB));
          td[(size_t)j * n + i] = v;
        }
        double g = 0.0, acc = 0.0;
        for (int k = 0; k < d; ++k) {
          double p[4];
          sde_coef(comp[k].kind, field(&comp[k], 2, td, n, i), field(&comp[k], 3, td, n, i), field(&comp[k], 4, td, n, i), dt, p);
          const double xv = transition(comp[k].kind, p, dt, xs[(size_t)k * n + a], filter_normal(key, i, r, CSSM_STREAM_STEP, d, k));
          xd[(size_t)k * n + i] = xv;
          /* gamma = f(x, t): per-leaf dot product, leaves summed left-nested */
          if (comp[k].idx == 0) acc = fco[k] * xv;
          else if (comp[k].f_kind != 0) acc = acc + fco[k] * xv;
          if (k + 1 == d || comp[k + 1].leaf != comp[k].leaf) g = (comp[k].leaf == 0) ? acc : g + acc;
        }
        if (weighted) {
          double raw = 0.0, sd = 0.0, c[4], cdf;
          if (scaled) { raw = td[(size_t)scale_slot * n + i]; sd = cssm_exp(raw); }
          cssm_obs_consts(obs, y[r], ypart, sd, raw, df, c, &cdf);
          double lw = cssm_obs_logdens(obs, yk, c, cdf, g);
          if (lw != lw) lw = -cssm_inf();
          w[i] = lw;
          if (cssm_order_key(lw) > kmax) kmax = cssm_order_key(lw);
          if (own_level) { const uint64_t kc = cssm_order_key(cssm_if2_level(obs, y[r], sd, df)); if (kc > kcmax) kcmax = kc; }
        }
      }
      tp = t[r];
      if (!weighted) {
        for (uint32_t i = 0; i < n; ++i) anc[i] = i;
      } else {
        const double gmax = cssm_order_unkey(kmax);
        if (!(gmax > -cssm_inf()) || !(gmax < cssm_inf())) { rc = -5; break; }
        const double ref = cssm_ref_choose(own_level ? cssm_order_unkey(kcmax) : cssm_if2_level(obs, y[r], 1.0, df), gmax);
        cssm_u128 S = cssm_u128_zero(), S2 = cssm_u128_zero();
        for (uint32_t i = 0; i < n; ++i) {
          w[i] = cssm_exp_le0(cssm_min_c(w[i] - ref, CSSM_REF_BELOW));
          S = cssm_u128_add(S, cssm_fix_from_unit(w[i]));
          S2 = cssm_u128_add(S2, cssm_fix_from_unit(w[i] * w[i]));
        }
        if (cssm_u128_is_zero(S)) { rc = -5; break; }
        ll = ll + ref + cssm_log(cssm_fix_to_double(S) / (double)n);
        {                                                       /* ess = floor(1 / sum (w / tot)^2), the filter's */
          const double tot = cssm_fix_to_double(S), tot2 = cssm_fix_to_double(S2);
          const double e = 1.0 / (tot2 / (tot * tot));
          ess = (e < 2147483647.0) ? (int32_t)(double)(long long)e : 2147483647;
        }
        /* systematic resampling: particle j owns the slots [cnt(C_{j-1}), cnt(C_j)); a slot no particle owns takes the last owner before it */
        const double totd = cssm_u128_to_double(S), u = cssm_if2_uniform(key, r);
        cssm_u128 run = cssm_u128_zero();
        uint32_t prev = 0;
        for (uint32_t i = 0; i < n; ++i) anc[i] = 0u;
        for (uint32_t j = 0; j < n; ++j) {
          run = cssm_u128_add(run, cssm_fix_from_unit(w[j]));
          uint64_t e = cssm_sys_count(cssm_u128_to_double(run) / totd, u, n);
          if (e > n) e = n;
          if (e > prev) { anc[prev] = j; prev = (uint32_t)e; }
        }
        uint32_t carry = 0;
        for (uint32_t s = 0; s < n; ++s) { carry = anc[s] > carry ? anc[s] : carry; anc[s] = carry; }
      }
      if (ll_t) ll_t[r] = ll;
      if (ess_t) ess_t[r] = ess;
    }
    if (rc) { if (fail_iter) *fail_iter = q; break; }
    const double* tf = th[T & 1u];
    for (int j = 0; j < nt; ++j) {
      for (uint32_t i = 0; i < n; ++i) { swarm[(size_t)j * n + i] = tf[(size_t)j * n + anc[i]]; tree[i] = swarm[(size_t)j * n + i]; }
      for (uint32_t cnt = n; cnt > 1u; cnt = (cnt + 1u) / 2u)   /* the pairwise tree over the particle index */
        for (uint32_t i = 0; 2u * i < cnt; ++i) tree[i] = tree[2u * i] + ((2u * i + 1u < cnt) ? tree[2u * i + 1u] : 0.0);
      mean[(size_t)q * nt + j] = tree[0] / (double)n;
    }
    ll_out[q] = ll;
    if (q + 1u == n_iters) {
      if (x_out) memcpy(x_out, x[T & 1u], (size_t)d * n * 8u);
      if (anc_out) memcpy(anc_out, anc, (size_t)n * 4u);
    }
  }
done:
  free(th[0]); free(th[1]); free(x[0]); free(x[1]); free(w); free(tree); free(anc);
  return rc;
}

/* the perturbation normal alone, for the tests that pin it */
double twin_if2_normal(uint64_t key, uint64_t i, uint32_t when, uint32_t j) { return cssm_if2_normal(key, i, when, j, CSSM_LOG_TAB); }
