/* cssm_intervals.hip.h -- the arithmetic of the exact two-rank selection behind cssm_pf_filter_intervals (cssm_intervals.hip), shared by
 * the kernels, the host and the sequential twin (tests/cpp/intervals_twin.c): plain C, integers only.
 *
 * A row of a cloud is n order keys (cssm_order_key: unsigned, ascending with the double).  A TARGET is one rank of that row (the lower
 * or the upper order statistic).  Its state is an inclusive key range [lo, hi] known to hold the element of that rank, the rank counted
 * inside the range, and the number of keys inside it.  A PASS reads the target's source once, counts the in-range keys in
 * CSSM_IV_BINS equal sub-ranges of [lo, hi] (width 2^shift, so a key's sub-range is a subtraction and a shift), and the PICK moves the
 * target to the sub-range that holds the rank: hi - lo loses CSSM_IV_BITS bits per pass, and CSSM_IV_ROUNDS passes end at one key.
 *
 *   HIST_KEYS   the pass reads the row's keys
 *   COMPACT     the pass reads the row's keys and also copies the in-range ones to the target's candidate buffer (at most
 *               cssm_iv_cand_max(n) of them); later passes read that buffer
 *   HIST_CAND   the pass reads the candidate buffer (filtered by the range)
 *   RECOMPACT   at most CSSM_IV_CAP candidates are in range, but the candidate buffer is longer than that: the pass reads it and
 *               copies the in-range ones to the target's SHORT candidate buffer (one workgroup reading a long buffer took 300 us)
 *   DONE_CAND   at most CSSM_IV_CAP candidates are in range: one workgroup finishes the same passes in LDS
 *   DONE_CAND2  the same, from the short buffer
 *   DONE_EQ     lo == hi: that key is the answer (ties of any size end here)
 *
 * Everything is a function of counts, which are exact integers whatever order the blocks add them in. */
#pragma once

#include <stdint.h>

#include "../../include/cssm_numerics.h"

#define CSSM_IV_BITS 11
#define CSSM_IV_BINS 2048u
#define CSSM_IV_CAP 4096u  /* candidates the finishing workgroup holds in LDS */
#define CSSM_IV_ROUNDS 6   /* ceil(64 / CSSM_IV_BITS): the passes enqueued per row */

#define CSSM_IV_DONE_EQ 0u
#define CSSM_IV_DONE_CAND 1u
#define CSSM_IV_DONE_CAND2 2u
#define CSSM_IV_HIST_KEYS 3u
#define CSSM_IV_COMPACT 4u
#define CSSM_IV_HIST_CAND 5u
#define CSSM_IV_RECOMPACT 6u

typedef struct {
  uint64_t lo, hi;   /* inclusive key range that holds the element */
  uint64_t rank;     /* its rank among the keys inside [lo, hi] (0-based, ascending) */
  uint64_t cnt;      /* keys inside [lo, hi] */
  uint64_t ncand;    /* entries of the candidate buffer (COMPACT has run) */
  uint32_t mode;
  uint32_t ncand2;   /* entries of the short candidate buffer (RECOMPACT has run): at most CSSM_IV_CAP */
} cssm_iv_target;

/* candidate slots per target: a quarter of the row, at least what the finishing workgroup holds */
CSSM_HD uint64_t cssm_iv_cand_max(uint64_t n) { return (n / 4u > CSSM_IV_CAP) ? n / 4u : (uint64_t)CSSM_IV_CAP; }

/* width of a sub-range of [lo, hi] as a shift: (hi - lo) >> shift < CSSM_IV_BINS */
CSSM_HD int cssm_iv_shift(uint64_t lo, uint64_t hi) {
  const uint64_t span = hi - lo;
  const int bits = span ? 64 - (int)__builtin_clzll((unsigned long long)span) : 0;
  return bits > CSSM_IV_BITS ? bits - CSSM_IV_BITS : 0;
}
CSSM_HD int cssm_iv_in(uint64_t k, uint64_t lo, uint64_t hi) { return (k - lo) <= (hi - lo); }
CSSM_HD uint32_t cssm_iv_bin(uint64_t k, uint64_t lo, int shift) { return (uint32_t)((k - lo) >> shift); }
CSSM_HD int cssm_iv_active(uint32_t mode) { return mode >= CSSM_IV_HIST_KEYS; }
CSSM_HD int cssm_iv_reads_cand(uint32_t mode) { return mode == CSSM_IV_HIST_CAND || mode == CSSM_IV_RECOMPACT; }
CSSM_HD int cssm_iv_reads_keys(uint32_t mode) { return mode == CSSM_IV_HIST_KEYS || mode == CSSM_IV_COMPACT; }

/* a row's target before its first pass: the whole row, between its smallest and largest key */
CSSM_HD cssm_iv_target cssm_iv_start(uint64_t kmin, uint64_t kmax, uint64_t rank, uint64_t n) {
  cssm_iv_target s;
  s.lo = kmin; s.hi = kmax; s.rank = rank; s.cnt = n; s.ncand = 0; s.ncand2 = 0;
  s.mode = (kmin == kmax) ? CSSM_IV_DONE_EQ : (n <= cssm_iv_cand_max(n) ? CSSM_IV_COMPACT : CSSM_IV_HIST_KEYS);
  return s;
}

/* the sub-range that holds rank: the first bin whose running count exceeds it; *below = the keys in the bins before it */
CSSM_HD uint32_t cssm_iv_pick(const uint32_t* hist, uint64_t rank, uint64_t* below) {
  uint64_t cum = 0;
  uint32_t b = 0;
  for (; b + 1u < CSSM_IV_BINS; ++b) {
    if (cum + hist[b] > rank) break;
    cum += hist[b];
  }
  *below = cum;
  return b;
}

/* the target after a pass: bin b holds the rank, `below` in-range keys lie in the bins before it, `c` in it; n = the row's size */
CSSM_HD cssm_iv_target cssm_iv_next(cssm_iv_target s, uint32_t b, uint64_t below, uint64_t c, uint64_t n) {
  const int shift = cssm_iv_shift(s.lo, s.hi);
  const uint64_t span = (shift >= 64) ? ~(uint64_t)0 : (((uint64_t)1 << shift) - 1u);
  const uint64_t nlo = s.lo + ((uint64_t)b << shift);
  const uint64_t nhi = (s.hi - nlo < span) ? s.hi : nlo + span;
  const int from_cand = s.mode == CSSM_IV_COMPACT || s.mode == CSSM_IV_HIST_CAND;
  const int recompacted = s.mode == CSSM_IV_RECOMPACT;
  if (s.mode == CSSM_IV_COMPACT) s.ncand = s.cnt;
  if (recompacted) s.ncand2 = (uint32_t)s.cnt;
  s.lo = nlo; s.hi = nhi; s.rank = s.rank - below; s.cnt = c;
  if (nlo == nhi) s.mode = CSSM_IV_DONE_EQ;
  else if (recompacted) s.mode = CSSM_IV_DONE_CAND2;
  else if (from_cand) s.mode = (c > CSSM_IV_CAP) ? CSSM_IV_HIST_CAND : (s.ncand <= CSSM_IV_CAP ? CSSM_IV_DONE_CAND : CSSM_IV_RECOMPACT);
  else s.mode = (c <= cssm_iv_cand_max(n)) ? CSSM_IV_COMPACT : CSSM_IV_HIST_KEYS;
  return s;
}

/* The two ranks of a row, 0-based in ascending order of a cloud of n (sel_ranks, cssm_kernels.hip.h): getCredibleInterval takes
 * (n - index - 1, index - 1) for a state row, getOrderStatistic (n - index, index) for eta, index = floor(interval n); clamped. */
CSSM_HD void cssm_iv_ranks(uint64_t n, double interval, int state_row, uint64_t* r_lower, uint64_t* r_upper) {
  const long long idx = (long long)__builtin_floor(interval * (double)n);
  long long a = state_row ? (long long)n - idx - 1 : (long long)n - idx, b = state_row ? idx - 1 : idx;
  if (a < 0) a = 0;
  if (a > (long long)n - 1) a = (long long)n - 1;
  if (b < 0) b = 0;
  if (b > (long long)n - 1) b = (long long)n - 1;
  *r_lower = (uint64_t)a; *r_upper = (uint64_t)b;
}
