/* backsim_twin.c -- a sequential statement of the contract's backward simulation (include/cssm_numerics.h, "backward simulation"),
 * written from that header alone (gcc -O2 -ffp-contract=off -mfma), loaded with ctypes by tests/test_fleet_smooth_host.py and
 * tests/test_gpu_fleet_smooth.py: the trajectories cssm_fleet_smooth draws through a given history.
 *
 * X    [T + 1][d][n]   slice 0 the initial cloud, slice s + 1 the cloud record s proposed
 * A    [T + 1][n]      the ancestors that resampled slice s (the caller writes the identity for s = 0 and behind an unweighted record)
 * recs [T][80 + 40 d]  the bytes of cssm_fleet_pack_record: 9 doubles (y, c[4], cdf, u, dt, ref), has_obs (i32), step (u32), then
 *                      d x 4 transition coefficients p0..p3 and d f coefficients
 * kind [d]             CSSM_SDE_* of every component
 * traj [T + 1][M]      out: the particle of slice s trajectory m passes through */
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/cssm_numerics.h"

int twin_backsim(const double* X, const uint32_t* A, const unsigned char* recs, const int32_t* kind, uint64_t seed, uint32_t n, uint32_t M,
                 uint32_t T, int d, uint32_t* traj) {
  const size_t RB = 80u + 40u * (size_t)d;
  double* lb = (double*)malloc((size_t)n * sizeof(double));
  if (!lb) return -1;
  for (uint32_t m = 0; m < M; ++m) {
    uint32_t j = A[(size_t)T * n + cssm_back_start(m, n, M)];
    traj[(size_t)T * M + m] = j;
    for (uint32_t s = T; s-- > 0u;) {
      const unsigned char* r = recs + (size_t)s * RB;
      double dt, coef[64];
      memcpy(&dt, r + 7 * 8, 8);
      memcpy(coef, r + 80, (size_t)d * 4u * 8u);
      const double* Xs = X + (size_t)s * d * n;
      const double* Xn = X + ((size_t)s + 1u) * d * n;
      const uint32_t* As = A + (size_t)s * n;
      int gen = 0;
      for (int c = 0; c < d; ++c)
        if (!(cssm_back_sd(kind[c], coef[4 * c + 2], coef[4 * c + 3]) > 0.0)) gen = 1;
      uint32_t is = j;
      if (!gen) {
        double level = -cssm_inf();
        for (uint32_t i = 0; i < n; ++i) {
          double q = 0.0;
          for (int c = 0; c < d; ++c) {
            const double mean = cssm_back_mean(kind[c], coef[4 * c], coef[4 * c + 1], dt, Xs[(size_t)c * n + As[i]]);
            const double e = (Xn[(size_t)c * n + j] - mean) / cssm_back_sd(kind[c], coef[4 * c + 2], coef[4 * c + 3]);
            q = q + e * e;
          }
          lb[i] = cssm_back_lb(q);
          if (lb[i] > level) level = lb[i];
        }
        if (level > -cssm_inf()) {
          cssm_u128 tot = cssm_u128_zero(), acc = cssm_u128_zero();
          for (uint32_t i = 0; i < n; ++i) tot = cssm_u128_add(tot, cssm_fix_from_unit(cssm_back_weight(lb[i], level)));
          const double totd = cssm_u128_to_double(tot);
          const double u = cssm_back_uniform(seed, m, s);
          is = n - 1u;
          for (uint32_t i = 0; i < n; ++i) {
            acc = cssm_u128_add(acc, cssm_fix_from_unit(cssm_back_weight(lb[i], level)));
            if (cssm_u128_to_double(acc) / totd >= u) { is = i; break; }
          }
        }
      }
      j = As[is];
      traj[(size_t)s * M + m] = j;
    }
  }
  free(lb);
  return 0;
}

/* the uniform and the start slot alone, for the tests that pin them */
double twin_back_uniform(uint64_t seed, uint32_t m, uint32_t s) { return cssm_back_uniform(seed, m, s); }
uint32_t twin_back_start(uint32_t m, uint32_t n, uint32_t M) { return cssm_back_start(m, n, M); }
