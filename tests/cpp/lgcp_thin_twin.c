/* lgcp_thin_twin.c -- the host build of the thinning statements of include/cssm_obs_draws.h (gcc -O2 -ffp-contract=off -mfma), loaded
 * with ctypes by tests/test_simulate_lgcp_host.py and tests/test_gpu_simulate_lgcp.py: the candidates, the index rule and the whole
 * candidate loop of one path, which the device must reproduce bit for bit. */
#include <stddef.h>
#include <stdint.h>

#include "../../include/cssm_obs_draws.h"

void twin_lgcp_candidate(uint64_t key, uint64_t i, uint32_t c, double ub, double* E, double* V) { cssm_lgcp_candidate(key, i, c, ub, E, V); }

uint32_t twin_lgcp_index(const double* grid_t, uint32_t n_grid, double start, double delta, double t1) {
  return cssm_lgcp_index(grid_t, n_grid, start, delta, t1);
}

/* The loop of path i from its eta column (eta[k] = the stored value of grid index k) and its bound ub.  Writes at most `cap` events
 * (time, grid index); returns the path's status, *n_events and *n_candidates as the device reports them. */
int twin_lgcp_thin(uint64_t key, uint64_t i, const double* grid_t, const double* eta, uint32_t n_grid, double start, double end, double delta,
                   double ub, double* ev_t, uint32_t* ev_idx, size_t cap, uint32_t* n_events, uint32_t* n_candidates) {
  int st = cssm_lgcp_admit(ub, start, end);
  uint32_t c = 0u, e = 0u;
  if (st == CSSM_LGCP_PATH_OK) {
    double last = start;
    for (;;) {
      double E, V;
      if (c == CSSM_LGCP_MAX_CANDIDATES) { st = CSSM_LGCP_PATH_TOO_MANY; break; }
      cssm_lgcp_candidate(key, i, c, ub, &E, &V);
      const double t1 = last + E;
      if (!(t1 <= end)) break;
      c += 1u;
      const uint32_t k = cssm_lgcp_index(grid_t, n_grid, start, delta, t1);
      if (V <= eta[k] / ub) {
        if (e < cap) { ev_t[e] = t1; ev_idx[e] = k; }
        e += 1u;
      }
      last = t1;
    }
  }
  *n_events = st == CSSM_LGCP_PATH_OK ? e : 0u;
  *n_candidates = c;
  return st;
}
