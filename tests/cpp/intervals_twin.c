/* intervals_twin.c -- a sequential statement of the two-rank selection behind cssm_pf_filter_intervals, written on the arithmetic the
 * kernels share with the host (composablestatespacemodels_amd/csrc/cssm_intervals.hip.h: ranges, sub-ranges, picks, when a target is
 * finished).  gcc -O2 -ffp-contract=off -mfma, loaded with ctypes by tests/test_filter_intervals_host.py and
 * tests/test_gpu_filter_intervals.py.  It walks one row the way the launches do -- the fill (keys, min, max), up to CSSM_IV_ROUNDS
 * passes over the keys or the compacted candidates for both targets, the finish on at most CSSM_IV_CAP candidates -- and reports what the
 * device's budget is counted from.
 *
 * x      [n]   the row
 * out    [2]   the elements of rank r_lower and r_upper (0-based, ascending)
 * stats  [8]   0: passes run (the last round either target was active in)   1: of those, passes that read the row's keys
 *              2, 3: candidates in range when target 0 / 1 finished (0: it ended on a range one key wide)
 *              4, 5: the targets' final modes   6: candidates compacted, both targets   7: passes of the finish, both targets
 * returns 0, or < 0: -1 no memory, -2 a compaction beyond the candidate buffer, -3 a target still active behind the enqueued passes,
 *              -4 more than CSSM_IV_CAP candidates at the finish */
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../../composablestatespacemodels_amd/csrc/cssm_intervals.hip.h"

int twin_iv_select(const double* x, uint64_t n, uint64_t r_lower, uint64_t r_upper, double* out, uint64_t* stats) {
  const uint64_t cand_max = cssm_iv_cand_max(n);
  uint64_t* keys = (uint64_t*)malloc((size_t)n * 8u);
  uint64_t* cand[2] = {(uint64_t*)malloc((size_t)cand_max * 8u), (uint64_t*)malloc((size_t)cand_max * 8u)};
  uint32_t* hist = (uint32_t*)malloc(2u * CSSM_IV_BINS * 4u);
  uint64_t* lds = (uint64_t*)malloc(CSSM_IV_CAP * 8u);
  uint64_t* cand2[2] = {(uint64_t*)malloc(CSSM_IV_CAP * 8u), (uint64_t*)malloc(CSSM_IV_CAP * 8u)};
  int rc = 0;
  memset(stats, 0, 8 * sizeof(uint64_t));
  if (!keys || !cand[0] || !cand[1] || !cand2[0] || !cand2[1] || !hist || !lds || n < 1) { rc = -1; goto done; }
  {
    uint64_t kmin = ~(uint64_t)0, kmax = 0, ccnt[2] = {0, 0}, ccnt2[2] = {0, 0};
    cssm_iv_target tg[2];
    for (uint64_t i = 0; i < n; ++i) {                                   /* the fill */
      keys[i] = cssm_order_key(x[i]);
      if (keys[i] < kmin) kmin = keys[i];
      if (keys[i] > kmax) kmax = keys[i];
    }
    tg[0] = cssm_iv_start(kmin, kmax, r_lower, n);
    tg[1] = cssm_iv_start(kmin, kmax, r_upper, n);
    for (int r = 1; r <= CSSM_IV_ROUNDS; ++r) {                          /* the enqueued passes */
      if (!cssm_iv_active(tg[0].mode) && !cssm_iv_active(tg[1].mode)) break;
      stats[0] = (uint64_t)r;
      memset(hist, 0, 2u * CSSM_IV_BINS * 4u);
      if (cssm_iv_reads_keys(tg[0].mode) || cssm_iv_reads_keys(tg[1].mode)) {
        stats[1]++;
        for (uint64_t i = 0; i < n; ++i)
          for (int t = 0; t < 2; ++t) {
            if (!cssm_iv_reads_keys(tg[t].mode) || !cssm_iv_in(keys[i], tg[t].lo, tg[t].hi)) continue;
            hist[t * CSSM_IV_BINS + cssm_iv_bin(keys[i], tg[t].lo, cssm_iv_shift(tg[t].lo, tg[t].hi))]++;
            if (tg[t].mode == CSSM_IV_COMPACT) {
              if (ccnt[t] >= cand_max) { rc = -2; goto done; }
              cand[t][ccnt[t]++] = keys[i];
            }
          }
      }
      for (int t = 0; t < 2; ++t) {
        if (!cssm_iv_reads_cand(tg[t].mode)) continue;
        for (uint64_t i = 0; i < tg[t].ncand; ++i)
          if (cssm_iv_in(cand[t][i], tg[t].lo, tg[t].hi)) {
            hist[t * CSSM_IV_BINS + cssm_iv_bin(cand[t][i], tg[t].lo, cssm_iv_shift(tg[t].lo, tg[t].hi))]++;
            if (tg[t].mode == CSSM_IV_RECOMPACT) {
              if (ccnt2[t] >= CSSM_IV_CAP) { rc = -4; goto done; }
              cand2[t][ccnt2[t]++] = cand[t][i];
            }
          }
      }
      for (int t = 0; t < 2; ++t) {
        uint64_t below;
        uint32_t b;
        if (!cssm_iv_active(tg[t].mode)) continue;
        b = cssm_iv_pick(hist + t * CSSM_IV_BINS, tg[t].rank, &below);
        tg[t] = cssm_iv_next(tg[t], b, below, hist[t * CSSM_IV_BINS + b], n);
      }
    }
    stats[6] = ccnt[0] + ccnt[1];
    for (int t = 0; t < 2; ++t) {                                        /* the finish */
      cssm_iv_target g = tg[t];
      stats[4 + t] = g.mode;
      if (cssm_iv_active(g.mode) && g.mode != CSSM_IV_RECOMPACT) { rc = -3; goto done; }
      if (g.mode == CSSM_IV_DONE_CAND || g.mode == CSSM_IV_DONE_CAND2 || g.mode == CSSM_IV_RECOMPACT) {   /* (RECOMPACT: no pass was left for it) */
        const uint64_t* src = g.mode == CSSM_IV_DONE_CAND2 ? cand2[t] : cand[t];
        const uint64_t len = g.mode == CSSM_IV_DONE_CAND2 ? g.ncand2 : g.ncand;
        uint64_t m = 0;
        if (g.ncand != ccnt[t] || (g.mode == CSSM_IV_DONE_CAND2 && g.ncand2 != ccnt2[t])) { rc = -2; goto done; }
        for (uint64_t i = 0; i < len; ++i)
          if (cssm_iv_in(src[i], g.lo, g.hi)) {
            if (m >= CSSM_IV_CAP) { rc = -4; goto done; }
            lds[m++] = src[i];
          }
        stats[2 + t] = m;
        g.mode = CSSM_IV_HIST_CAND;
        for (int pass = 0; pass < CSSM_IV_ROUNDS && g.lo != g.hi; ++pass) {
          uint64_t below;
          uint32_t b;
          memset(hist, 0, CSSM_IV_BINS * 4u);
          for (uint64_t i = 0; i < m; ++i)
            if (cssm_iv_in(lds[i], g.lo, g.hi)) hist[cssm_iv_bin(lds[i], g.lo, cssm_iv_shift(g.lo, g.hi))]++;
          b = cssm_iv_pick(hist, g.rank, &below);
          g = cssm_iv_next(g, b, below, hist[b], n);
          g.mode = CSSM_IV_HIST_CAND;
          stats[7]++;
        }
        if (g.lo != g.hi) { rc = -3; goto done; }
      }
      out[t] = cssm_order_unkey(g.lo);
    }
  }
done:
  free(keys); free(cand[0]); free(cand[1]); free(cand2[0]); free(cand2[1]); free(hist); free(lds);
  return rc;
}

/* sel_ranks' rule as the library's host code applies it */
void twin_iv_ranks(uint64_t n, double interval, int state_row, uint64_t* r2) { cssm_iv_ranks(n, interval, state_row, &r2[0], &r2[1]); }

/* the constants a test states its bounds with: bins, cap, enqueued passes, candidate slots of a row of n */
void twin_iv_constants(uint64_t n, uint64_t* c4) {
  c4[0] = CSSM_IV_BINS; c4[1] = CSSM_IV_CAP; c4[2] = CSSM_IV_ROUNDS; c4[3] = cssm_iv_cand_max(n);
}
