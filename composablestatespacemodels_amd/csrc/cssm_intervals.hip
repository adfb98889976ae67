// cssm_intervals.hip -- the rows a batch filter of ONE large cloud forms between its observations: filtered intervals behind every record,
// one-step-ahead forecasts before every record (below), both on one exact two-rank selection.
// cssm_pf_filter_intervals, cssm_pf_filter_intervals_more, cssm_pf_step_intervals (include/cssm_pf.h): the
// filtered intervals of ONE large cloud, a row per observation, enqueued between the observations of the batch filter with no host
// round trip.  A row has the bits of cssm_pf_summary at that moment of the loop init; summary; (step; summary)*.
//
// Per row, on the handle's stream, 8 launches (cssm_pf_summary: 19) and no allocation:
//   k_iv_fill<D>        k_summary_fill's body and geometry (grid_for(n, CSSM_BLOCK, 1024) blocks, grid-stride, the wave butterfly: the
//                       means keep their bits): the order keys of the d state rows and of eta, the blocks' partial sums, and per block
//                       and row the smallest and the largest key.  Its blocks also clear the row's histograms and slot counters.
//   k_iv_round x 6      blocks (part of the row, row).  Every block first DERIVES the row's two targets (cssm_intervals.hip.h) from what
//                       the launch before left: the blocks' min / max (round 1) or the previous round's histogram and the targets block 0
//                       of that launch stored -- integer work on 16 KiB, the same in every block, so no block waits for another and the
//                       launch boundary is the only synchronisation.  Then one pass over the target's source: a histogram of the
//                       in-range keys over 2048 equal sub-ranges in LDS, merged with integer atomics; a COMPACT pass also copies the
//                       in-range keys to the target's candidate buffer (slots from an atomic counter, one add per block and 2048 keys:
//                       the order of the candidates depends on arrival, the multiset does not, and only counts of it reach an output).
//                       Later passes read the candidates; once at most CSSM_IV_CAP of a long buffer are in range one more pass copies
//                       them to a short buffer (RECOMPACT).  A row whose targets are both finished returns at once: after round 2
//                       or 3 that is the ordinary case.
//   k_iv_finish         a block per row: the last derivation; a target with at most CSSM_IV_CAP candidates in range runs the remaining
//                       passes in LDS; the mean by k_summary_finish's sequential combine; the row into the call's row buffer.
// The cloud is read once (fill), its keys twice in the ordinary case (round 1: histogram between min and max; round 2: compaction of the
// picked sub-range): 3 reads against 9.  A row whose picked sub-range holds more than a quarter of the row AND more than one key
// (heavy ties next to other values) reads its keys again, at most CSSM_IV_ROUNDS times in all.
// A series on hold (Scalars::err bit 6) or waiting for its second run: every kernel returns at once, as the filter's own do.
//
// cssm_pf_filter_forecasts, cssm_pf_filter_forecasts_more, cssm_pf_step_forecast: the one-step-ahead forecast of every record's time
// from the cloud BEFORE the record, a row enqueued in front of the record's own launches.  A row has the bits of
// cssm_pf_forecast(pf, &t[s], 1, key_s, ...) issued at that moment.  Per row 8 launches (cssm_pf_forecast: 18, with eight
// allocations, three events and a blocking read-back) and no allocation:
//   k_forecast_row<D>   (cssm_forecast.hip) forecast_body in k_forecast's geometry -- one thread per particle pair, no cap on the blocks,
//                       the blocks' partial sums of all d + 2 rows: the means keep their bits --: transition, gamma, eta, the observation
//                       draw, the order keys; per block and row the smallest and the largest key, per block the two PIT counts; its
//                       blocks clear the row's histograms and slot counters.
//   k_iv_round x 6      the selection above over d + 2 rows; the observation row takes eta's ranks (getOrderStatistic).
//   k_fc_finish         a block per row: the last derivation and the remaining passes in LDS; EVERY row's mean by k_forecast_finish's
//                       combine (thread-strided over the blocks, the wave butterfly, the waves in order); the PIT counts added up.
// The cloud is read once (through its ancestors), its keys twice in the ordinary case of a state or eta row.  An observation row of
// counts (Poisson at rate 2: about ten distinct keys; Bernoulli: two) is the heavy-ties case above as a matter of course: its keys are
// read again, at most CSSM_IV_ROUNDS times.  The records the rows move under are StepRecs of their own (horizon index 0), uploaded with
// the call; under a hold the rows behind the held record return at once and are enqueued again with the records, the held record's
// own row was formed before the hold and stands.
#include <hip/hip_runtime.h>

#include <cmath>
#include <vector>

#include "cssm_internal.h"
#include "cssm_kernels.hip.h"
#include "cssm_intervals.hip.h"

#define IV_ITEMS 8
#define IV_CHUNK (CSSM_BLOCK * IV_ITEMS)   /* keys a block reads per iteration */
#define IV_PART_KEYS 16384                 /* keys per block of a pass: a block merges its histogram with up to 2 x 2048 atomics, so not too few */
#define IV_MAX_PARTS 128                   /* blocks per row of a pass */

struct IvRow { cssm_iv_target tg[2]; };

struct IvArgs {
  const unsigned long long* keys;   // [rows][n]
  uint64_t n;
  int rows, d, nblocks;             // rows: d + 1, or a forecast's d + 2; nblocks: the grid of k_iv_fill, or of k_forecast_row
  const unsigned long long* pmm;    // [nblocks][rows][2]: the blocks' min and max key
  const double* partial;            // [nblocks][d] (a forecast: [nblocks][rows])
  uint32_t* hist;                   // [CSSM_IV_ROUNDS][rows][2][CSSM_IV_BINS]
  uint32_t* ccnt;                   // [2][rows][2]: candidate slots handed out, of the long and of the short buffer
  unsigned long long* cand;         // [rows][2][cand_max]
  unsigned long long* cand2;        // [rows][2][CSSM_IV_CAP]: the short buffers (RECOMPACT)
  uint64_t cand_max;
  IvRow* st;                        // [CSSM_IV_ROUNDS][rows]: the targets the round launches derived
  uint64_t rank[4];                 // state row lower, upper; eta row lower, upper
  const Scalars* sc;
};

__device__ __forceinline__ unsigned long long iv_shfl_xor(unsigned long long v, int off) {
  const uint32_t lo = __shfl_xor((uint32_t)v, off, 64), hi = __shfl_xor((uint32_t)(v >> 32), off, 64);
  return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ uint32_t iv_wave_incl_scan(uint32_t v) {
  const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) { const uint32_t o = __shfl_up(v, off, 64); if (lane >= (uint32_t)off) v += o; }
  return v;
}

template <int D>
__global__ __launch_bounds__(CSSM_BLOCK) void k_iv_fill(const double* __restrict__ src, size_t src_stride, const uint32_t* __restrict__ anc,
                                                        uint64_t n, const double* __restrict__ fco, ModelK mk,
                                                        unsigned long long* __restrict__ keys, double* __restrict__ partial /*[gridDim.x][D]*/,
                                                        unsigned long long* __restrict__ pmm /*[gridDim.x][D + 1][2]*/,
                                                        uint32_t* __restrict__ zero, size_t zero_words, const Scalars* __restrict__ sc,
                                                        unsigned long long* __restrict__ stamp) {
  __shared__ double s_p[CSSM_BLOCK / 64][D];
  __shared__ unsigned long long s_mm[CSSM_BLOCK / 64][D + 1][2];
  if (sc->err & IV_HELD) return;
  if (blockIdx.x == 0 && threadIdx.x == 0) stamp[0] = __builtin_amdgcn_s_memrealtime();
  for (size_t w = (size_t)blockIdx.x * CSSM_BLOCK + threadIdx.x; w < zero_words; w += (size_t)gridDim.x * CSSM_BLOCK) zero[w] = 0u;
  double acc[D];
  unsigned long long kmin[D + 1], kmax[D + 1];
#pragma unroll
  for (int k = 0; k < D; ++k) acc[k] = 0.0;
#pragma unroll
  for (int k = 0; k <= D; ++k) { kmin[k] = ~0ull; kmax[k] = 0ull; }
  for (uint64_t i = (uint64_t)blockIdx.x * CSSM_BLOCK + threadIdx.x; i < n; i += (uint64_t)gridDim.x * CSSM_BLOCK) {
    const size_t j = anc ? (size_t)anc[i] : (size_t)i;
    double x[D];
#pragma unroll
    for (int k = 0; k < D; ++k) {
      x[k] = src[(size_t)k * src_stride + j];
      const unsigned long long key = cssm_order_key(x[k]);
      keys[(size_t)k * n + i] = key;
      kmin[k] = key < kmin[k] ? key : kmin[k]; kmax[k] = key > kmax[k] ? key : kmax[k];
      acc[k] += x[k];
    }
    const unsigned long long key = cssm_order_key(link_of(mk.obs_kind, gamma_coef<D>(mk, fco, x)));
    keys[(size_t)D * n + i] = key;
    kmin[D] = key < kmin[D] ? key : kmin[D]; kmax[D] = key > kmax[D] ? key : kmax[D];
  }
#pragma unroll
  for (int k = 0; k < D; ++k) {
    double v = acc[k];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    if ((threadIdx.x & 63) == 0) s_p[threadIdx.x >> 6][k] = v;
  }
#pragma unroll
  for (int k = 0; k <= D; ++k) {
    unsigned long long a = kmin[k], b = kmax[k];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const unsigned long long oa = iv_shfl_xor(a, off), ob = iv_shfl_xor(b, off);
      a = oa < a ? oa : a; b = ob > b ? ob : b;
    }
    if ((threadIdx.x & 63) == 0) { s_mm[threadIdx.x >> 6][k][0] = a; s_mm[threadIdx.x >> 6][k][1] = b; }
  }
  __syncthreads();
  if (threadIdx.x < D) {
    double v = 0.0;
    for (int w = 0; w < CSSM_BLOCK / 64; ++w) v += s_p[w][threadIdx.x];
    partial[(size_t)blockIdx.x * D + threadIdx.x] = v;
  }
  if (threadIdx.x <= D) {
    unsigned long long a = ~0ull, b = 0ull;
    for (int w = 0; w < CSSM_BLOCK / 64; ++w) {
      const unsigned long long oa = s_mm[w][threadIdx.x][0], ob = s_mm[w][threadIdx.x][1];
      a = oa < a ? oa : a; b = ob > b ? ob : b;
    }
    pmm[((size_t)blockIdx.x * (D + 1) + threadIdx.x) * 2] = a;
    pmm[((size_t)blockIdx.x * (D + 1) + threadIdx.x) * 2 + 1] = b;
  }
}

// cssm_pf_step_interpolate: k_compose and k_iv_fill in one launch -- row j of the call summarises slice (newest - j) of the handle's window
// through the lineages that survive to the newest cloud.  X: the slice's cloud (rows `stride` apart), A: the ancestors that resampled it
// (null, a slice without a datum: none did), b: the lineage composed so far, one index per slot, read and written by the slot's own thread
// alone (b_in = b; null for row 0, which starts from the identity -- so b carries nothing from one call to the next): j = A[b[i]], left in
// b[i] for the row of the slice before.  Everything else is k_iv_fill's body, grid, loop and reduction order, line for line: the means keep
// cssm_pf_summary's bits.  (A kernel of its own, not a flag of k_iv_fill: that kernel's code is the parent's, instruction for instruction.)
template <int D>
__global__ __launch_bounds__(CSSM_BLOCK) void k_lineage_fill(const double* __restrict__ X, size_t stride, const uint32_t* __restrict__ A,
                                                             const uint32_t* b_in, uint32_t* b, uint64_t n, const double* __restrict__ fco, ModelK mk,
                                                             unsigned long long* __restrict__ keys, double* __restrict__ partial /*[gridDim.x][D]*/,
                                                             unsigned long long* __restrict__ pmm /*[gridDim.x][D + 1][2]*/,
                                                             uint32_t* __restrict__ zero, size_t zero_words, const Scalars* __restrict__ sc,
                                                             unsigned long long* __restrict__ stamp) {
  __shared__ double s_p[CSSM_BLOCK / 64][D];
  __shared__ unsigned long long s_mm[CSSM_BLOCK / 64][D + 1][2];
  if (sc->err & IV_HELD) return;
  if (blockIdx.x == 0 && threadIdx.x == 0) stamp[0] = __builtin_amdgcn_s_memrealtime();
  for (size_t w = (size_t)blockIdx.x * CSSM_BLOCK + threadIdx.x; w < zero_words; w += (size_t)gridDim.x * CSSM_BLOCK) zero[w] = 0u;
  double acc[D];
  unsigned long long kmin[D + 1], kmax[D + 1];
#pragma unroll
  for (int k = 0; k < D; ++k) acc[k] = 0.0;
#pragma unroll
  for (int k = 0; k <= D; ++k) { kmin[k] = ~0ull; kmax[k] = 0ull; }
  for (uint64_t i = (uint64_t)blockIdx.x * CSSM_BLOCK + threadIdx.x; i < n; i += (uint64_t)gridDim.x * CSSM_BLOCK) {
    uint32_t q = b_in ? b_in[i] : (uint32_t)i;
    if (A) q = A[q];
    b[i] = q;
    const size_t j = (size_t)q;
    double x[D];
#pragma unroll
    for (int k = 0; k < D; ++k) {
      x[k] = X[(size_t)k * stride + j];
      const unsigned long long key = cssm_order_key(x[k]);
      keys[(size_t)k * n + i] = key;
      kmin[k] = key < kmin[k] ? key : kmin[k]; kmax[k] = key > kmax[k] ? key : kmax[k];
      acc[k] += x[k];
    }
    const unsigned long long key = cssm_order_key(link_of(mk.obs_kind, gamma_coef<D>(mk, fco, x)));
    keys[(size_t)D * n + i] = key;
    kmin[D] = key < kmin[D] ? key : kmin[D]; kmax[D] = key > kmax[D] ? key : kmax[D];
  }
#pragma unroll
  for (int k = 0; k < D; ++k) {
    double v = acc[k];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    if ((threadIdx.x & 63) == 0) s_p[threadIdx.x >> 6][k] = v;
  }
#pragma unroll
  for (int k = 0; k <= D; ++k) {
    unsigned long long a = kmin[k], c = kmax[k];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const unsigned long long oa = iv_shfl_xor(a, off), ob = iv_shfl_xor(c, off);
      a = oa < a ? oa : a; c = ob > c ? ob : c;
    }
    if ((threadIdx.x & 63) == 0) { s_mm[threadIdx.x >> 6][k][0] = a; s_mm[threadIdx.x >> 6][k][1] = c; }
  }
  __syncthreads();
  if (threadIdx.x < D) {
    double v = 0.0;
    for (int w = 0; w < CSSM_BLOCK / 64; ++w) v += s_p[w][threadIdx.x];
    partial[(size_t)blockIdx.x * D + threadIdx.x] = v;
  }
  if (threadIdx.x <= D) {
    unsigned long long a = ~0ull, c = 0ull;
    for (int w = 0; w < CSSM_BLOCK / 64; ++w) {
      const unsigned long long oa = s_mm[w][threadIdx.x][0], ob = s_mm[w][threadIdx.x][1];
      a = oa < a ? oa : a; c = ob > c ? ob : c;
    }
    pmm[((size_t)blockIdx.x * (D + 1) + threadIdx.x) * 2] = a;
    pmm[((size_t)blockIdx.x * (D + 1) + threadIdx.x) * 2 + 1] = c;
  }
}

// A cloud into a slot of the window: row k of the slot is row k of `src` -- gathered through `gather` for the base slice (the cloud as
// cssm_pf_get_particles returns it), as it is for the cloud a step proposed --, and where ancestors resampled it (anc_src) they go beside
// it.  Returns at once on a held series, like the step's own kernels: the slice is put again behind the redo.
__global__ __launch_bounds__(256) void k_slice_put(const double* __restrict__ src, size_t src_stride, const uint32_t* __restrict__ gather,
                                                   const uint32_t* __restrict__ anc_src, uint64_t n, int d, double* __restrict__ dst,
                                                   size_t dst_stride, uint32_t* __restrict__ anc_dst, const Scalars* __restrict__ sc) {
  if (sc->err & IV_HELD) return;
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
    const size_t j = gather ? (size_t)gather[i] : (size_t)i;
    for (int k = 0; k < d; ++k) dst[(size_t)k * dst_stride + i] = src[(size_t)k * src_stride + j];
    if (anc_src) anc_dst[i] = anc_src[i];
  }
}

// what the block's LDS holds beside the histograms
struct IvShared {
  uint32_t part[CSSM_BLOCK];
  unsigned long long res[3];                       // the pick: bin, keys below it, keys in it
  unsigned long long red[CSSM_BLOCK / 64][2];
  uint32_t w[2][CSSM_BLOCK / 64];
  uint32_t base[2];
};

// cssm_iv_pick by the whole block over a histogram in LDS: every thread returns the same (bin, below, count)
__device__ __forceinline__ void iv_block_pick(const uint32_t* h, uint64_t rank, IvShared& s, uint32_t& bin, uint64_t& below, uint64_t& cnt) {
  const uint32_t tid = threadIdx.x, lane = tid & 63u;
  constexpr uint32_t PER = CSSM_IV_BINS / CSSM_BLOCK;          // 8 bins per thread
  uint32_t sum = 0;
#pragma unroll
  for (uint32_t j = 0; j < PER; ++j) sum += h[tid * PER + j];
  s.part[tid] = sum;
  __syncthreads();
  if (tid < 64u) {                                             // wave 0: lane l owns the 32 bins [32 l, 32 l + 32)
    uint32_t q = 0;
#pragma unroll
    for (uint32_t j = 0; j < CSSM_BLOCK / 64; ++j) q += s.part[lane * (CSSM_BLOCK / 64) + j];
    const uint64_t incl = (uint64_t)iv_wave_incl_scan(q);      // (counts of one row: below 2^32)
    const unsigned long long hit = __ballot(incl > rank);
    const uint32_t first = hit ? (uint32_t)__builtin_ctzll(hit) : 63u;
    if (lane == first) {
      uint64_t cum = incl - q;
      uint32_t b = lane * 32u;
      for (; b + 1u < CSSM_IV_BINS && b < lane * 32u + 32u; ++b) {
        if (cum + h[b] > rank) break;
        cum += h[b];
      }
      if (b >= CSSM_IV_BINS) b = CSSM_IV_BINS - 1u;
      s.res[0] = b; s.res[1] = cum; s.res[2] = h[b];
    }
  }
  __syncthreads();
  bin = (uint32_t)s.res[0]; below = s.res[1]; cnt = s.res[2];
  __syncthreads();
}

// The row's targets as the launch `r` finds them (r = 0: from the fill's min / max; r >= 1: the targets launch r stored, moved by the
// histogram launch r added up).  Every thread of every block of the row returns the same value.  s_h: [2][CSSM_IV_BINS] of LDS.
__device__ __forceinline__ IvRow iv_derive(const IvArgs& a, int r, int row, uint32_t* s_h, IvShared& s) {
  const uint32_t tid = threadIdx.x;
  IvRow S;
  if (r == 0) {
    unsigned long long mn = ~0ull, mx = 0ull;
    for (int b = (int)tid; b < a.nblocks; b += CSSM_BLOCK) {
      const unsigned long long oa = a.pmm[((size_t)b * a.rows + row) * 2], ob = a.pmm[((size_t)b * a.rows + row) * 2 + 1];
      mn = oa < mn ? oa : mn; mx = ob > mx ? ob : mx;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const unsigned long long oa = iv_shfl_xor(mn, off), ob = iv_shfl_xor(mx, off);
      mn = oa < mn ? oa : mn; mx = ob > mx ? ob : mx;
    }
    if ((tid & 63u) == 0u) { s.red[tid >> 6][0] = mn; s.red[tid >> 6][1] = mx; }
    __syncthreads();
    mn = ~0ull; mx = 0ull;
    for (int w = 0; w < CSSM_BLOCK / 64; ++w) { mn = s.red[w][0] < mn ? s.red[w][0] : mn; mx = s.red[w][1] > mx ? s.red[w][1] : mx; }
    __syncthreads();
    const int e = row >= a.d ? 2 : 0;   // (eta, and a forecast's observation row behind it: getOrderStatistic's ranks)
    S.tg[0] = cssm_iv_start(mn, mx, a.rank[e], a.n);
    S.tg[1] = cssm_iv_start(mn, mx, a.rank[e + 1], a.n);
    return S;
  }
  S = a.st[(size_t)(r - 1) * a.rows + row];
  const uint32_t* H = a.hist + (((size_t)(r - 1) * a.rows + row) * 2) * CSSM_IV_BINS;
  const bool act0 = cssm_iv_active(S.tg[0].mode), act1 = cssm_iv_active(S.tg[1].mode);
  if (!act0 && !act1) return S;
  for (uint32_t i = tid; i < 2u * CSSM_IV_BINS; i += CSSM_BLOCK) s_h[i] = ((i < CSSM_IV_BINS) ? act0 : act1) ? H[i] : 0u;
  __syncthreads();
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    if (!cssm_iv_active(S.tg[t].mode)) continue;               // (uniform)
    uint32_t bin; uint64_t below, cnt;
    iv_block_pick(s_h + t * CSSM_IV_BINS, S.tg[t].rank, s, bin, below, cnt);
    S.tg[t] = cssm_iv_next(S.tg[t], bin, below, cnt, a.n);
  }
  return S;
}

// pass r (1 .. CSSM_IV_ROUNDS) of every row: grid (parts, rows)
__global__ __launch_bounds__(CSSM_BLOCK) void k_iv_round(const IvArgs a, int r) {
  __shared__ uint32_t s_h[2 * CSSM_IV_BINS];
  __shared__ IvShared s;
  if (a.sc->err & IV_HELD) return;
  const int row = blockIdx.y;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wid = tid >> 6;
  const IvRow S = iv_derive(a, r - 1, row, s_h, s);
  if (blockIdx.x == 0 && tid == 0) a.st[(size_t)(r - 1) * a.rows + row] = S;
  const uint32_t m0 = S.tg[0].mode, m1 = S.tg[1].mode;
  if (!cssm_iv_active(m0) && !cssm_iv_active(m1)) return;      // (uniform) the row is finished
  __syncthreads();
  for (uint32_t i = tid; i < 2u * CSSM_IV_BINS; i += CSSM_BLOCK) s_h[i] = 0u;
  __syncthreads();
  const uint64_t lo[2] = {S.tg[0].lo, S.tg[1].lo}, hi[2] = {S.tg[0].hi, S.tg[1].hi};
  const int sh[2] = {cssm_iv_shift(lo[0], hi[0]), cssm_iv_shift(lo[1], hi[1])};
  // (both targets on one range -- the first pass of a large row: one histogram, merged into both)
  const bool twin = m0 == CSSM_IV_HIST_KEYS && m1 == CSSM_IV_HIST_KEYS && lo[0] == lo[1] && hi[0] == hi[1];
  const bool rk[2] = {(bool)cssm_iv_reads_keys(m0), cssm_iv_reads_keys(m1) && !twin};
  const bool cp[2] = {m0 == CSSM_IV_COMPACT, m1 == CSSM_IV_COMPACT};
  if (rk[0] || rk[1]) {
    const unsigned long long* kr = a.keys + (size_t)row * a.n;
    const uint64_t nch = (a.n + IV_CHUNK - 1) / IV_CHUNK;
    for (uint64_t ch = blockIdx.x; ch < nch; ch += gridDim.x) {    // (uniform)
      unsigned long long k[IV_ITEMS];
      bool v[IV_ITEMS];
#pragma unroll
      for (int j = 0; j < IV_ITEMS; ++j) {
        const uint64_t i = ch * IV_CHUNK + (uint64_t)j * CSSM_BLOCK + tid;
        v[j] = i < a.n;
        k[j] = v[j] ? kr[i] : 0ull;
      }
      uint32_t m[2] = {0u, 0u}, inm[2] = {0u, 0u};
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        if (!rk[t]) continue;
#pragma unroll
        for (int j = 0; j < IV_ITEMS; ++j)
          if (v[j] && cssm_iv_in(k[j], lo[t], hi[t])) {
            atomicAdd(&s_h[t * CSSM_IV_BINS + cssm_iv_bin(k[j], lo[t], sh[t])], 1u);
            inm[t] |= 1u << j; ++m[t];
          }
      }
      if (cp[0] || cp[1]) {                                        // (uniform) slots for the block's in-range keys: one add per target
        uint32_t pre[2] = {0u, 0u};
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          if (!cp[t]) continue;
          const uint32_t incl = iv_wave_incl_scan(m[t]);
          if (lane == 63u) s.w[t][wid] = incl;
          pre[t] = incl - m[t];
        }
        __syncthreads();
        if (tid < 2u && (tid == 0u ? cp[0] : cp[1])) {
          uint32_t tot = 0;
          for (int w = 0; w < CSSM_BLOCK / 64; ++w) tot += s.w[tid][w];
          s.base[tid] = tot ? atomicAdd(&a.ccnt[row * 2 + tid], tot) : 0u;
        }
        __syncthreads();
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          if (!cp[t]) continue;
          uint64_t off = (uint64_t)s.base[t] + pre[t];
          for (uint32_t w = 0; w < wid; ++w) off += s.w[t][w];
          unsigned long long* cb = a.cand + ((size_t)row * 2 + t) * a.cand_max;
#pragma unroll
          for (int j = 0; j < IV_ITEMS; ++j)
            if ((inm[t] >> j) & 1u) { if (off < a.cand_max) cb[off] = k[j]; ++off; }
        }
        __syncthreads();
      }
    }
  }
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    if (!cssm_iv_reads_cand(t ? m1 : m0)) continue;                // (uniform)
    const bool re = (t ? m1 : m0) == CSSM_IV_RECOMPACT;            // at most CSSM_IV_CAP keys are in range: a slot each in the short buffer
    const unsigned long long* cb = a.cand + ((size_t)row * 2 + t) * a.cand_max;
    unsigned long long* cb2 = a.cand2 + ((size_t)row * 2 + t) * CSSM_IV_CAP;
    const uint64_t len = S.tg[t].ncand < a.cand_max ? S.tg[t].ncand : a.cand_max;
    for (uint64_t i = (uint64_t)blockIdx.x * CSSM_BLOCK + tid; i < len; i += (uint64_t)gridDim.x * CSSM_BLOCK) {
      const unsigned long long key = cb[i];
      if (cssm_iv_in(key, lo[t], hi[t])) {
        atomicAdd(&s_h[t * CSSM_IV_BINS + cssm_iv_bin(key, lo[t], sh[t])], 1u);
        if (re) { const uint32_t q = atomicAdd(&a.ccnt[(a.rows + row) * 2 + t], 1u); if (q < CSSM_IV_CAP) cb2[q] = key; }
      }
    }
  }
  __syncthreads();
  uint32_t* H = a.hist + (((size_t)(r - 1) * a.rows + row) * 2) * CSSM_IV_BINS;
  for (uint32_t i = tid; i < 2u * CSSM_IV_BINS; i += CSSM_BLOCK) {
    const uint32_t c = s_h[(twin && i >= CSSM_IV_BINS) ? i - CSSM_IV_BINS : i];
    if (c) atomicAdd(&H[i], c);
  }
}

// The two selected keys of a row behind its last pass, by the row's one block: the last derivation, and a target with at most CSSM_IV_CAP
// candidates in range runs its remaining passes in LDS (s_h: [2][CSSM_IV_BINS], s_k: [CSSM_IV_CAP]).  Ends on a block barrier.
__device__ __forceinline__ void iv_final_keys(const IvArgs& a, int row, uint32_t* s_h, IvShared& s, unsigned long long* s_k, uint32_t& s_m,
                                              unsigned long long (&key)[2]) {
  const uint32_t tid = threadIdx.x;
  const IvRow S = iv_derive(a, CSSM_IV_ROUNDS, row, s_h, s);
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    cssm_iv_target g = S.tg[t];
    // (RECOMPACT: no pass was left for it -- the long buffer then, by this one block)
    if (g.mode == CSSM_IV_DONE_CAND || g.mode == CSSM_IV_DONE_CAND2 || g.mode == CSSM_IV_RECOMPACT) {   // (uniform) the in-range candidates into LDS, the remaining passes there
      __syncthreads();
      if (tid == 0) s_m = 0u;
      __syncthreads();
      const bool shortbuf = g.mode == CSSM_IV_DONE_CAND2;
      const unsigned long long* cb = shortbuf ? a.cand2 + ((size_t)row * 2 + t) * CSSM_IV_CAP : a.cand + ((size_t)row * 2 + t) * a.cand_max;
      const uint64_t len = shortbuf ? (g.ncand2 < CSSM_IV_CAP ? g.ncand2 : CSSM_IV_CAP) : (g.ncand < a.cand_max ? g.ncand : a.cand_max);
      for (uint64_t i = tid; i < len; i += CSSM_BLOCK) {
        const unsigned long long c = cb[i];
        if (cssm_iv_in(c, g.lo, g.hi)) { const uint32_t q = atomicAdd(&s_m, 1u); if (q < CSSM_IV_CAP) s_k[q] = c; }
      }
      __syncthreads();
      const uint32_t m = s_m < CSSM_IV_CAP ? s_m : CSSM_IV_CAP;
      g.mode = CSSM_IV_HIST_CAND;
      for (int pass = 0; pass < CSSM_IV_ROUNDS && g.lo != g.hi; ++pass) {   // (uniform)
        for (uint32_t i = tid; i < CSSM_IV_BINS; i += CSSM_BLOCK) s_h[i] = 0u;
        __syncthreads();
        const int sh = cssm_iv_shift(g.lo, g.hi);
        for (uint32_t i = tid; i < m; i += CSSM_BLOCK)
          if (cssm_iv_in(s_k[i], g.lo, g.hi)) atomicAdd(&s_h[cssm_iv_bin(s_k[i], g.lo, sh)], 1u);
        __syncthreads();
        uint32_t bin; uint64_t below, cnt;
        iv_block_pick(s_h, g.rank, s, bin, below, cnt);
        g = cssm_iv_next(g, bin, below, cnt, a.n);
        g.mode = CSSM_IV_HIST_CAND;
      }
      key[t] = g.lo;
    } else {
      key[t] = (g.mode == CSSM_IV_DONE_EQ) ? g.lo : cssm_order_key(cssm_nan());   // (every target is finished after CSSM_IV_ROUNDS passes)
    }
  }
  __syncthreads();
}

// the row: one block per row of the cloud
__global__ __launch_bounds__(CSSM_BLOCK) void k_iv_finish(const IvArgs a, double* __restrict__ out /*[3][rows]: mean, lower, upper*/,
                                                          unsigned long long* __restrict__ stamp /*[0] the fill's start, [1] ticks so far*/) {
  __shared__ uint32_t s_h[2 * CSSM_IV_BINS];
  __shared__ IvShared s;
  __shared__ unsigned long long s_k[CSSM_IV_CAP];
  __shared__ double s_part[1024];                                 // the fill's partial sums of this row (its grid: at most 1024 blocks)
  __shared__ uint32_t s_m;
  if (a.sc->err & IV_HELD) return;
  const int row = blockIdx.x;
  const uint32_t tid = threadIdx.x;
  // (the whole block fetches the partial sums: one thread adding them up straight from memory waited for 1024 loads in turn, 400 us)
  if (row < a.d) for (int b = (int)tid; b < a.nblocks && b < 1024; b += CSSM_BLOCK) s_part[b] = a.partial[(size_t)b * a.d + row];
  unsigned long long key[2];
  iv_final_keys(a, row, s_h, s, s_k, s_m, key);
  if (tid == 0) {
    if (row < a.d) {
      double sum = 0.0;                                           // k_summary_finish's sequential combine over the blocks
#pragma unroll 8
      for (int b = 0; b < a.nblocks && b < 1024; ++b) sum += s_part[b];
      out[row] = sum / (double)a.n;
    } else {
      out[row] = 0.0;   // eta of the mean state is formed on the host: link(f(mean, t))
    }
    out[a.rows + row] = cssm_order_unkey(key[0]);
    out[2 * a.rows + row] = cssm_order_unkey(key[1]);
    if (row == 0) stamp[1] += __builtin_amdgcn_s_memrealtime() - stamp[0];
  }
}

// The row of a one-step-ahead forecast (cssm_pf_filter_forecasts): one block per row of the d + 2.  Every row has a mean, formed as
// k_forecast_finish (cssm_forecast.hip) combines the partial sums of k_forecast's blocks -- thread-strided over the blocks, the wave
// butterfly, the waves in order --; the block of the observation row also adds up the blocks' PIT counts (integers).
__global__ __launch_bounds__(CSSM_BLOCK) void k_fc_finish(const IvArgs a, const uint32_t* __restrict__ pit /*[nblocks][2]*/,
                                                          double* __restrict__ out /*[3][rows]: mean, lower, upper; then the two counts (int32)*/,
                                                          unsigned long long* __restrict__ stamp) {
  __shared__ uint32_t s_h[2 * CSSM_IV_BINS];
  __shared__ IvShared s;
  __shared__ unsigned long long s_k[CSSM_IV_CAP];
  __shared__ double s_w[CSSM_BLOCK / 64];
  __shared__ uint32_t s_c[2];
  __shared__ uint32_t s_m;
  if (a.sc->err & IV_HELD) return;
  const int row = blockIdx.x;
  const uint32_t tid = threadIdx.x;
  if (tid < 2u) s_c[tid] = 0u;
  double v = 0.0;
  for (int b = (int)tid; b < a.nblocks; b += CSSM_BLOCK) v += a.partial[(size_t)b * a.rows + row];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  if ((tid & 63u) == 0u) s_w[tid >> 6] = v;
  __syncthreads();
  if (row == a.rows - 1) {                                        // (uniform)
    uint32_t c0 = 0u, c1 = 0u;
    for (int b = (int)tid; b < a.nblocks; b += CSSM_BLOCK) { c0 += pit[(size_t)b * 2]; c1 += pit[(size_t)b * 2 + 1]; }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { c0 += __shfl_xor(c0, off, 64); c1 += __shfl_xor(c1, off, 64); }
    if ((tid & 63u) == 0u) { atomicAdd(&s_c[0], c0); atomicAdd(&s_c[1], c1); }
  }
  unsigned long long key[2];
  iv_final_keys(a, row, s_h, s, s_k, s_m, key);
  if (tid == 0) {
    double sum = 0.0;
    for (int w = 0; w < CSSM_BLOCK / 64; ++w) sum += s_w[w];
    out[row] = sum / (double)a.n;
    out[a.rows + row] = cssm_order_unkey(key[0]);
    out[2 * a.rows + row] = cssm_order_unkey(key[1]);
    if (row == a.rows - 1) {
      int32_t* cnt = reinterpret_cast<int32_t*>(out + 3 * (size_t)a.rows);
      cnt[0] = (int32_t)s_c[0]; cnt[1] = (int32_t)s_c[1];
    }
    if (row == 0) stamp[1] += __builtin_amdgcn_s_memrealtime() - stamp[0];
  }
}

// ------------------------------------------------------------------------------------ host side
// The selection's scratch lives on the handle: made at the first call, the per-call parts grown on demand, freed with the handle.  One
// per kind of row: cssm_pf::iv (filtered intervals, d + 1 rows from k_iv_fill) and cssm_pf::fc (forecasts, d + 2 rows from k_forecast_row).
struct IvScratch {
  unsigned long long *keys = nullptr, *pmm = nullptr, *cand = nullptr, *cand2 = nullptr, *stamp = nullptr;
  double *partial = nullptr, *fco = nullptr, *rows = nullptr, *h_rows = nullptr;
  uint32_t* zero = nullptr;      // the histograms, then the slot counters
  IvRow* st = nullptr;
  size_t zero_words = 0, fco_cap = 0, rows_cap = 0;
  size_t out_stride = 0;         // doubles per row of the call's row buffer: 3 per row of the cloud (a forecast: + 1, its two PIT counts)
  uint64_t cand_max = 0;
  int nblocks = 0;
  uint64_t rank[4] = {0, 0, 0, 0};
  std::vector<double> h_fco;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  bool timed = false;
  double ms[2] = {-1.0, -1.0};
  // forecasts: the blocks' PIT counts; the call's records (apart from the filter's), and per record its key, its datum and whether
  // cssm_pf_forecast would refuse its time (no launch, a NaN row)
  uint32_t* pit = nullptr;
  StepRec* recs = nullptr;
  std::vector<StepRec> h_recs;
  std::vector<uint64_t> key;
  std::vector<double> y;
  std::vector<uint8_t> has, refused;
};

static void iv_free_one(void*& slot) {
  IvScratch* s = static_cast<IvScratch*>(slot);
  if (!s) return;
  void* ptrs[] = {s->keys, s->pmm, s->cand, s->cand2, s->stamp, s->partial, s->fco, s->rows, s->zero, s->st, s->pit, s->recs};
  for (void* p : ptrs) if (p) (void)hipFree(p);
  if (s->h_rows) (void)hipHostFree(s->h_rows);
  if (s->ev0) (void)hipEventDestroy(s->ev0);
  if (s->ev1) (void)hipEventDestroy(s->ev1);
  delete s;
  slot = nullptr;
}
static void window_free(cssm_pf* pf);
void cssm_iv_free(cssm_pf* pf) {
  iv_free_one(pf->iv);
  iv_free_one(pf->fc);
  iv_free_one(pf->li);
  window_free(pf);
}

#define IV_ALLOC(p, bytes)                                                                                               \
  do {                                                                                                                   \
    void* q__ = nullptr;                                                                                                 \
    if (hipMalloc(&q__, (bytes)) != hipSuccess) return fail(CSSM_ENOMEM, "hipMalloc(%zu) for " #p, (size_t)(bytes));     \
    p = static_cast<decltype(p)>(q__);                                                                                   \
  } while (0)

// scratch (the handle's `slot`) for calls of up to nrows rows; the ranks of `interval`.  fc: rows of a forecast -- d + 2 of them, the first
// launch in k_forecast's geometry (one thread per particle pair, no cap on the blocks: the partial sums are the forecast's)
static int iv_ensure(cssm_pf* pf, void*& slot, bool fc, size_t nrows, double interval) {
  if (!slot) slot = new IvScratch();
  IvScratch* s = static_cast<IvScratch*>(slot);
  const int d = pf->d, rows = fc ? d + 2 : d + 1;
  const uint64_t n = pf->n;
  s->out_stride = 3 * (size_t)rows + (fc ? 1 : 0);
  if (!s->keys) {
    // (an earlier attempt that ran out of memory half way: start over)
    void** part[] = {(void**)&s->pmm, (void**)&s->partial, (void**)&s->cand, (void**)&s->cand2, (void**)&s->zero, (void**)&s->st, (void**)&s->stamp,
                     (void**)&s->pit};
    for (void** p : part) if (*p) { (void)hipFree(*p); *p = nullptr; }
    s->nblocks = fc ? (int)(((n + 1) / 2 + CSSM_BLOCK - 1) / CSSM_BLOCK) : grid_for(n, CSSM_BLOCK, 1024);
    s->cand_max = cssm_iv_cand_max(n);
    s->zero_words = (size_t)CSSM_IV_ROUNDS * rows * 2 * CSSM_IV_BINS + (size_t)rows * 4;
    IV_ALLOC(s->pmm, (size_t)s->nblocks * rows * 2 * 8);
    IV_ALLOC(s->partial, (size_t)s->nblocks * (fc ? rows : d) * 8);
    if (fc) IV_ALLOC(s->pit, (size_t)s->nblocks * 2 * 4);
    IV_ALLOC(s->cand, (size_t)rows * 2 * s->cand_max * 8);
    IV_ALLOC(s->cand2, (size_t)rows * 2 * CSSM_IV_CAP * 8);
    IV_ALLOC(s->zero, s->zero_words * 4);
    IV_ALLOC(s->st, (size_t)CSSM_IV_ROUNDS * rows * sizeof(IvRow));
    IV_ALLOC(s->stamp, 16);
    if (!s->ev0) HIP_TRY(hipEventCreate(&s->ev0));
    if (!s->ev1) HIP_TRY(hipEventCreate(&s->ev1));
    IV_ALLOC(s->keys, (size_t)rows * n * 8);                    // (last: its presence says the fixed part is complete)
  }
  if (s->fco_cap < nrows) {
    HIP_TRY(hipStreamSynchronize(pf->stream));
    if (s->fco) (void)hipFree(s->fco);
    if (s->rows) (void)hipFree(s->rows);
    if (s->recs) (void)hipFree(s->recs);
    if (s->h_rows) (void)hipHostFree(s->h_rows);
    s->fco = s->rows = s->h_rows = nullptr; s->recs = nullptr; s->fco_cap = s->rows_cap = 0;
    const size_t cap = nrows < 1024 ? 1024 : nrows + nrows / 2;
    if (fc) IV_ALLOC(s->recs, cap * sizeof(StepRec));
    else IV_ALLOC(s->fco, cap * CSSM_MAX_DIM * 8);
    IV_ALLOC(s->rows, cap * s->out_stride * 8);
    HIP_TRY(hipHostMalloc((void**)&s->h_rows, cap * s->out_stride * 8 + 16, hipHostMallocDefault));
    s->fco_cap = s->rows_cap = cap;
  }
  cssm_iv_ranks(n, interval, 1, &s->rank[0], &s->rank[1]);
  cssm_iv_ranks(n, interval, 0, &s->rank[2], &s->rank[3]);
  return CSSM_OK;
}

// The summary of the handle's current cloud, enqueued as row `row` of the call (its f coefficients: row `row` of the call's table).
// the selection's arguments over the `rows` rows of the scratch `s`, and its passes behind the row's first launch
static IvArgs iv_args(const cssm_pf* pf, const IvScratch* s, int rows) {
  IvArgs a;
  a.keys = s->keys; a.n = pf->n; a.rows = rows; a.d = pf->d; a.nblocks = s->nblocks; a.pmm = s->pmm; a.partial = s->partial;
  a.hist = s->zero; a.ccnt = s->zero + (size_t)CSSM_IV_ROUNDS * rows * 2 * CSSM_IV_BINS; a.cand = s->cand; a.cand2 = s->cand2; a.cand_max = s->cand_max;
  a.st = s->st; a.sc = pf->sc;
  for (int q = 0; q < 4; ++q) a.rank[q] = s->rank[q];
  return a;
}
static void iv_launch_rounds(cssm_pf* pf, const IvArgs& a) {
  const uint64_t parts64 = (a.n + IV_PART_KEYS - 1) / IV_PART_KEYS;
  const int parts = (int)(parts64 < 1 ? 1 : (parts64 > IV_MAX_PARTS ? IV_MAX_PARTS : parts64));
  for (int r = 1; r <= CSSM_IV_ROUNDS; ++r) hipLaunchKernelGGL(k_iv_round, dim3(parts, a.rows), dim3(CSSM_BLOCK), 0, pf->stream, a, r);
}

int cssm_iv_row(cssm_pf* pf, size_t row) {
  IvScratch* s = static_cast<IvScratch*>(pf->iv);
  if (!s || !s->keys || row >= s->rows_cap) return fail(CSSM_ESTATE, "a row of filtered intervals outside the call's row buffer");
  const int d = pf->d, rows = d + 1;
  const uint64_t n = pf->n;
  const IvArgs a = iv_args(pf, s, rows);
  DISPATCH_D(d, k_iv_fill<D><<<dim3(s->nblocks), dim3(CSSM_BLOCK), 0, pf->stream>>>(
                    pf->src, pf->src_stride, pf->anc_valid ? pf->anc : nullptr, n, s->fco + row * CSSM_MAX_DIM, pf->mk, s->keys, s->partial,
                    s->pmm, s->zero, s->zero_words, pf->sc, s->stamp));
  iv_launch_rounds(pf, a);
  hipLaunchKernelGGL(k_iv_finish, dim3(rows), dim3(CSSM_BLOCK), 0, pf->stream, a, s->rows + row * s->out_stride, s->stamp);
  HIP_TRY(hipGetLastError());
  return CSSM_OK;
}

// The forecast of record `row` of the running call from the cloud as the host-side source fields describe it now, enqueued as that row.
int cssm_fc_row(cssm_pf* pf, size_t row) {
  IvScratch* s = static_cast<IvScratch*>(pf->fc);
  if (!s || !s->keys || row >= s->rows_cap || row >= s->refused.size()) return fail(CSSM_ESTATE, "a forecast row outside the call's row buffer");
  if (s->refused[row]) return CSSM_OK;   // (a time cssm_pf_forecast refuses from this cloud: a NaN row, made by the host)
  const int rows = pf->d + 2;
  const IvArgs a = iv_args(pf, s, rows);
  const int rc = cssm_forecast_row_launch(pf, s->recs + row, s->key[row], s->y[row], s->has[row], s->keys, s->partial, s->pmm, s->pit, s->zero,
                                          s->zero_words, s->stamp, s->nblocks);
  if (rc) return rc;
  iv_launch_rounds(pf, a);
  hipLaunchKernelGGL(k_fc_finish, dim3(rows), dim3(CSSM_BLOCK), 0, pf->stream, a, (const uint32_t*)s->pit, s->rows + row * s->out_stride, s->stamp);
  HIP_TRY(hipGetLastError());
  return CSSM_OK;
}

// Behind the call's last launch: the end of its device time, and the rows (with the summaries' ticks) on their way to the host.
static int iv_results(cssm_pf* pf, IvScratch* s, size_t nrows) {
  HIP_TRY(hipEventRecord(s->ev1, pf->stream));
  HIP_TRY(hipMemcpyAsync(s->h_rows, s->rows, nrows * s->out_stride * 8, hipMemcpyDeviceToHost, pf->stream));
  HIP_TRY(hipMemcpyAsync(s->h_rows + s->rows_cap * s->out_stride, s->stamp, 16, hipMemcpyDeviceToHost, pf->stream));
  return CSSM_OK;
}
int cssm_iv_results(cssm_pf* pf, size_t nrows) { return iv_results(pf, static_cast<IvScratch*>(pf->iv), nrows); }
int cssm_fc_results(cssm_pf* pf, size_t nrows) { return iv_results(pf, static_cast<IvScratch*>(pf->fc), nrows); }

// what every call checks before any work, in its neighbours' words
static int iv_refuse(cssm_pf* pf, double interval) {
  if (!(interval > 0.0 && interval <= 1.0)) return fail(CSSM_EINVAL_ARG, "interval must be in (0, 1]");
  if (pf->sharded) return fail(CSSM_ESTATE, "a sharded handle is driven through the cssm_pf_shard_* stages");
  return CSSM_OK;
}

// the call's table of f coefficients, one row of CSSM_MAX_DIM per summary: F(t) of the row's time, as cssm_pf_summary builds it
static int iv_begin(cssm_pf* pf, const std::vector<double>& times, double interval) {
  HIP_TRY(hipSetDevice(pf->device));
  int rc = iv_ensure(pf, pf->iv, false, times.size(), interval);
  if (rc) return rc;
  IvScratch* s = static_cast<IvScratch*>(pf->iv);
  s->h_fco.assign(times.size() * CSSM_MAX_DIM, 0.0);
  StepRec hrec;
  for (size_t r = 0; r < times.size(); ++r) {
    cssm_build_rec(pf, times[r], times[r], 0.0, 0, pf->step, &hrec);
    memcpy(&s->h_fco[r * CSSM_MAX_DIM], hrec.fco, sizeof hrec.fco);
  }
  HIP_TRY(hipMemcpyAsync(s->fco, s->h_fco.data(), s->h_fco.size() * 8, hipMemcpyHostToDevice, pf->stream));
  HIP_TRY(hipMemsetAsync(s->stamp, 0, 16, pf->stream));
  s->timed = false; s->ms[0] = s->ms[1] = -1.0;
  HIP_TRY(hipEventRecord(s->ev0, pf->stream));
  return CSSM_OK;
}

// the downloaded rows -> the caller's arrays
static void iv_unpack(cssm_pf* pf, IvScratch* s, size_t nrows, double* state_mean, double* state_lower, double* state_upper, double* eta_of_mean,
                      double* eta_lower, double* eta_upper) {
  const int d = pf->d, rows = d + 1;
  for (size_t r = 0; r < nrows; ++r) {
    const double* h = s->h_rows + r * s->out_stride;
    for (int k = 0; k < d; ++k) {
      if (state_mean) state_mean[r * d + k] = h[k];
      if (state_lower) state_lower[r * d + k] = h[rows + k];
      if (state_upper) state_upper[r * d + k] = h[2 * rows + k];
    }
    if (eta_lower) eta_lower[r] = h[rows + d];
    if (eta_upper) eta_upper[r] = h[2 * rows + d];
    if (eta_of_mean) eta_of_mean[r] = cssm_eta_of_mean(*pf, &s->h_fco[r * CSSM_MAX_DIM], h);   // meanEta = link(f(stateMean, t)), :420
  }
  s->timed = true;
}

static int iv_filter(cssm_pf* pf, const double* t, const double* y, const uint8_t* has_obs, size_t T, double interval, bool cont,
                     double* ll_out, double* ll_t, int32_t* ess_t, double* state_mean, double* state_lower, double* state_upper,
                     double* eta_of_mean, double* eta_lower, double* eta_upper) {
  if (!pf || !t || !y) return fail(CSSM_EINVAL_ARG, "null argument");
  if (T < 1) return fail(CSSM_EINVAL_ARG, "empty data (the reference's minBy throws on an empty Vector)");
  int rc = iv_refuse(pf, interval);
  if (rc) return rc;
  if (cont && !pf->initialised) return fail(CSSM_ESTATE, "continuing a filter needs an initialised handle (and records no path)");
  std::vector<double> times;
  times.reserve(T + 1);
  if (!cont) times.push_back(cssm_series_t0(t, T));
  times.insert(times.end(), t, t + T);
  rc = iv_begin(pf, times, interval);
  if (rc) return rc;
  rc = cssm_run_filter_rows(pf, t, y, has_obs, T, ll_out, ll_t, ess_t, cont);
  if (rc) return rc;
  iv_unpack(pf, static_cast<IvScratch*>(pf->iv), times.size(), state_mean, state_lower, state_upper, eta_of_mean, eta_lower, eta_upper);
  return CSSM_OK;
}

extern "C" int cssm_pf_filter_intervals(cssm_pf* pf, const double* t, const double* y, const uint8_t* has_obs, size_t T, double interval,
                                        double* ll_out, double* ll_t, int32_t* ess_t, double* state_mean, double* state_lower,
                                        double* state_upper, double* eta_of_mean, double* eta_lower, double* eta_upper) {
  return iv_filter(pf, t, y, has_obs, T, interval, false, ll_out, ll_t, ess_t, state_mean, state_lower, state_upper, eta_of_mean, eta_lower, eta_upper);
}

extern "C" int cssm_pf_filter_intervals_more(cssm_pf* pf, const double* t, const double* y, const uint8_t* has_obs, size_t T, double interval,
                                             double* ll_out, double* ll_t, int32_t* ess_t, double* state_mean, double* state_lower,
                                             double* state_upper, double* eta_of_mean, double* eta_lower, double* eta_upper) {
  return iv_filter(pf, t, y, has_obs, T, interval, true, ll_out, ll_t, ess_t, state_mean, state_lower, state_upper, eta_of_mean, eta_lower, eta_upper);
}

extern "C" int cssm_pf_step_intervals(cssm_pf* pf, double t, double obs, int has_obs, double interval, double* ll_out, int32_t* ess_out,
                                      double* state_mean, double* state_lower, double* state_upper, double* eta_of_mean, double* eta_lower,
                                      double* eta_upper) {
  if (!pf) return fail(CSSM_EINVAL_ARG, "null handle");
  if (!pf->initialised) return fail(CSSM_ESTATE, "cssm_pf_step before cssm_pf_init");
  int rc = iv_refuse(pf, interval);
  if (rc) return rc;
  rc = iv_begin(pf, std::vector<double>(1, t), interval);
  if (rc) return rc;
  rc = cssm_step_rows(pf, t, obs, has_obs, ll_out, ess_out);
  if (rc) return rc;
  iv_unpack(pf, static_cast<IvScratch*>(pf->iv), 1, state_mean, state_lower, state_upper, eta_of_mean, eta_lower, eta_upper);
  return CSSM_OK;
}

// the device times of the last completed call on the scratch `s`: the event pair, and the ticks its rows' launches added up
static int iv_last_ms(cssm_pf* pf, IvScratch* s, double* ms2, const char* what) {
  if (!s || !s->timed) return fail(CSSM_ESTATE, "no call of %s has completed on this handle", what);
  if (s->ms[0] < 0.0) {
    HIP_TRY(hipSetDevice(pf->device));
    float ms = 0.f;
    HIP_TRY(hipEventSynchronize(s->ev1));
    HIP_TRY(hipEventElapsedTime(&ms, s->ev0, s->ev1));
    unsigned long long ticks = 0;
    memcpy(&ticks, reinterpret_cast<const char*>(s->h_rows + s->rows_cap * s->out_stride) + 8, 8);
    s->ms[0] = (double)ms;
    s->ms[1] = (double)ticks * 1e-5;   // 100 MHz
  }
  ms2[0] = s->ms[0]; ms2[1] = s->ms[1];
  return CSSM_OK;
}

extern "C" int cssm_pf_intervals_last_ms(cssm_pf* pf, double* ms2) {
  if (!pf || !ms2) return fail(CSSM_EINVAL_ARG, "null argument");
  return iv_last_ms(pf, static_cast<IvScratch*>(pf->iv), ms2, "filtered intervals");
}

// ------------------------------------------------------------------------------------ one-step-ahead forecasts
// The call's forecast records, apart from the filter's: record s moves the cloud before it over t[s] - (the time before it) at horizon
// index 0, as forecast_chunks builds the one record of cssm_pf_forecast(&t[s], 1); its key, its datum (for the PIT counts) and whether
// cssm_pf_forecast would refuse its time (cssm_check_times: not finite, or before the cloud's time).  t_prev: the time before record 0;
// base: the observation index of the cloud before record 0.
static int fc_begin(cssm_pf* pf, const double* t, const double* y, const uint8_t* has, size_t T, const uint64_t* keys, double interval,
                    double t_prev, uint32_t base) {
  HIP_TRY(hipSetDevice(pf->device));
  int rc = iv_ensure(pf, pf->fc, true, T, interval);
  if (rc) return rc;
  IvScratch* s = static_cast<IvScratch*>(pf->fc);
  s->h_recs.resize(T); s->key.resize(T); s->y.resize(T); s->has.resize(T); s->refused.resize(T);
  for (size_t r = 0; r < T; ++r) {
    const double tp = r ? t[r - 1] : t_prev;
    s->refused[r] = !(std::isfinite(t[r]) && t[r] >= tp);
    if (!s->refused[r]) cssm_build_rec(pf, tp, t[r], 0.0, 0, 0, &s->h_recs[r]);
    else memset(&s->h_recs[r], 0, sizeof(StepRec));
    s->key[r] = keys ? keys[r] : cssm_pf_run_key(pf->seed, (1ull << 63) | (uint64_t)(base + (uint32_t)r));
    s->has[r] = has ? (has[r] != 0) : 1;
    s->y[r] = y[r];
  }
  HIP_TRY(hipMemcpyAsync(s->recs, s->h_recs.data(), T * sizeof(StepRec), hipMemcpyHostToDevice, pf->stream));
  HIP_TRY(hipMemsetAsync(s->stamp, 0, 16, pf->stream));
  s->timed = false; s->ms[0] = s->ms[1] = -1.0;
  HIP_TRY(hipEventRecord(s->ev0, pf->stream));
  return CSSM_OK;
}

struct FcOut {
  double *state_mean, *state_lower, *state_upper, *eta_mean, *eta_lower, *eta_upper, *obs_mean, *obs_lower, *obs_upper;
  int32_t *obs_below, *obs_equal;
};

// the downloaded rows -> the caller's arrays (a refused time: NaN and -1; a record without a datum: counts of -1)
static void fc_unpack(cssm_pf* pf, size_t nrows, const FcOut& o) {
  IvScratch* s = static_cast<IvScratch*>(pf->fc);
  const int d = pf->d, rows = d + 2;
  std::vector<double> nan_row(s->out_stride, cssm_nan());
  for (size_t r = 0; r < nrows; ++r) {
    const bool bad = s->refused[r] != 0;
    const double* h = bad ? nan_row.data() : s->h_rows + r * s->out_stride;
    for (int k = 0; k < d; ++k) {
      if (o.state_mean) o.state_mean[r * d + k] = h[k];
      if (o.state_lower) o.state_lower[r * d + k] = h[rows + k];
      if (o.state_upper) o.state_upper[r * d + k] = h[2 * rows + k];
    }
    if (o.eta_mean) o.eta_mean[r] = h[d];
    if (o.eta_lower) o.eta_lower[r] = h[rows + d];
    if (o.eta_upper) o.eta_upper[r] = h[2 * rows + d];
    if (o.obs_mean) o.obs_mean[r] = h[d + 1];
    if (o.obs_lower) o.obs_lower[r] = h[rows + d + 1];
    if (o.obs_upper) o.obs_upper[r] = h[2 * rows + d + 1];
    int32_t cnt[2] = {-1, -1};
    if (!bad && s->has[r]) memcpy(cnt, h + 3 * (size_t)rows, 8);
    if (o.obs_below) o.obs_below[r] = cnt[0];
    if (o.obs_equal) o.obs_equal[r] = cnt[1];
  }
  s->timed = true;
}

static int fc_filter(cssm_pf* pf, const double* t, const double* y, const uint8_t* has_obs, size_t T, const uint64_t* keys, double interval, bool cont,
                     double* ll_out, double* ll_t, int32_t* ess_t, const FcOut& o) {
  if (!pf || !t || !y) return fail(CSSM_EINVAL_ARG, "null argument");
  if (T < 1) return fail(CSSM_EINVAL_ARG, "empty data (the reference's minBy throws on an empty Vector)");
  int rc = iv_refuse(pf, interval);
  if (rc) return rc;
  if (cont && !pf->initialised) return fail(CSSM_ESTATE, "continuing a filter needs an initialised handle (and records no path)");
  rc = cssm_forecast_refuse_model(pf);
  if (rc) return rc;
  rc = fc_begin(pf, t, y, has_obs, T, keys, interval, cont ? pf->t : cssm_series_t0(t, T), cont ? pf->step : 0u);
  if (rc) return rc;
  rc = cssm_run_filter_rows(pf, t, y, has_obs, T, ll_out, ll_t, ess_t, cont, CSSM_ROWS_FORECASTS);
  if (rc) return rc;
  fc_unpack(pf, T, o);
  return CSSM_OK;
}

extern "C" int cssm_pf_filter_forecasts(cssm_pf* pf, const double* t, const double* y, const uint8_t* has_obs, size_t T, const uint64_t* keys,
                                        double interval, double* ll_out, double* ll_t, int32_t* ess_t, double* state_mean, double* state_lower,
                                        double* state_upper, double* eta_mean, double* eta_lower, double* eta_upper, double* obs_mean,
                                        double* obs_lower, double* obs_upper, int32_t* obs_below, int32_t* obs_equal) {
  return fc_filter(pf, t, y, has_obs, T, keys, interval, false, ll_out, ll_t, ess_t,
                   FcOut{state_mean, state_lower, state_upper, eta_mean, eta_lower, eta_upper, obs_mean, obs_lower, obs_upper, obs_below, obs_equal});
}

extern "C" int cssm_pf_filter_forecasts_more(cssm_pf* pf, const double* t, const double* y, const uint8_t* has_obs, size_t T, const uint64_t* keys,
                                             double interval, double* ll_out, double* ll_t, int32_t* ess_t, double* state_mean,
                                             double* state_lower, double* state_upper, double* eta_mean, double* eta_lower, double* eta_upper,
                                             double* obs_mean, double* obs_lower, double* obs_upper, int32_t* obs_below, int32_t* obs_equal) {
  return fc_filter(pf, t, y, has_obs, T, keys, interval, true, ll_out, ll_t, ess_t,
                   FcOut{state_mean, state_lower, state_upper, eta_mean, eta_lower, eta_upper, obs_mean, obs_lower, obs_upper, obs_below, obs_equal});
}

extern "C" int cssm_pf_step_forecast(cssm_pf* pf, double t, double obs, int has_obs, uint64_t key, int use_key, double interval, double* ll_out,
                                     int32_t* ess_out, double* state_mean, double* state_lower, double* state_upper, double* eta_mean,
                                     double* eta_lower, double* eta_upper, double* obs_mean, double* obs_lower, double* obs_upper,
                                     int32_t* obs_below, int32_t* obs_equal) {
  if (!pf) return fail(CSSM_EINVAL_ARG, "null handle");
  if (!(interval > 0.0 && interval <= 1.0)) return fail(CSSM_EINVAL_ARG, "interval must be in (0, 1]");
  if (pf->sharded) return fail(CSSM_ESTATE, "a sharded handle is driven through the cssm_pf_shard_* stages");
  if (!pf->initialised) return fail(CSSM_ESTATE, "cssm_pf_step before cssm_pf_init");
  int rc = cssm_forecast_refuse_model(pf);
  if (rc) return rc;
  const uint8_t has = has_obs ? 1 : 0;
  rc = fc_begin(pf, &t, &obs, &has, 1, use_key ? &key : nullptr, interval, pf->t, pf->step);
  if (rc) return rc;
  rc = cssm_step_rows(pf, t, obs, has_obs, ll_out, ess_out, CSSM_ROWS_FORECASTS);
  if (rc) return rc;
  fc_unpack(pf, 1, FcOut{state_mean, state_lower, state_upper, eta_mean, eta_lower, eta_upper, obs_mean, obs_lower, obs_upper, obs_below, obs_equal});
  return CSSM_OK;
}

extern "C" int cssm_pf_forecasts_last_ms(cssm_pf* pf, double* ms2) {
  if (!pf || !ms2) return fail(CSSM_EINVAL_ARG, "null argument");
  return iv_last_ms(pf, static_cast<IvScratch*>(pf->fc), ms2, "one-step-ahead forecasts");
}

// ------------------------------------------------------------------------------------ fixed-lag lineages of a live handle
// cssm_pf_window / cssm_pf_step_interpolate (include/cssm_pf.h): FilterInterpolate as the stream it is, for ONE large cloud.  The handle
// keeps a ring of its `slices` most recent clouds and of the ancestors that resampled them; cssm_pf_step_interpolate is cssm_pf_step, a
// copy of the cloud the step proposed into the ring (k_slice_put, behind the step's launches) and, for the last lag + 1 time indices, a
// row each of 8 launches: k_lineage_fill, the selection's six passes, k_iv_finish.  Which slot is which: cssm_window.h.
struct PfWindow {
  double* X = nullptr;          // [slices][d][stride]: the clouds
  uint32_t* A = nullptr;        // [slices][stride]: the ancestors that resampled them (where weighted)
  uint32_t* b = nullptr;        // [n]: the lineage composed so far, within one call
  std::vector<double> time;     // per slot: the slice's time
  std::vector<uint8_t> weighted;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  uint32_t nrows = 0;           // rows of the running (then of the last completed) call
  bool timed = false;
  unsigned long long ticks = 0;
  double ms0 = -1.0;
};

static void window_free(cssm_pf* pf) {
  PfWindow* W = static_cast<PfWindow*>(pf->win);
  cssm_window_open(&pf->wring, 0u);
  if (!W) return;
  if (W->X) (void)hipFree(W->X);
  if (W->A) (void)hipFree(W->A);
  if (W->b) (void)hipFree(W->b);
  if (W->ev0) (void)hipEventDestroy(W->ev0);
  if (W->ev1) (void)hipEventDestroy(W->ev1);
  delete W;
  pf->win = nullptr;
}

// what cssm_pf_window and cssm_pf_step_interpolate refuse of the handle itself
static int li_refuse_handle(const cssm_pf* pf) {
  if (pf->sharded) return fail(CSSM_ESTATE, "a sharded handle is driven through the cssm_pf_shard_* stages");
  if (pf->obs_kind == CSSM_OBS_LGCP) return fail(CSSM_EINVAL_ARG, "FilterInterpolate weighs with dataLikelihood; the LGCP filter has no path variant");
  return CSSM_OK;
}

extern "C" int cssm_pf_window(cssm_pf* pf, uint32_t slices) {
  if (!pf) return fail(CSSM_EINVAL_ARG, "null handle");
  int rc = li_refuse_handle(pf);
  if (rc) return rc;
  if (slices == 1u) return fail(CSSM_EINVAL_ARG, "a window holds at least 2 slices (the base slice and a record); 0 frees it");
  HIP_TRY(hipSetDevice(pf->device));
  if (pf->win) { HIP_TRY(hipStreamSynchronize(pf->stream)); window_free(pf); }
  if (slices == 0u) return CSSM_OK;
  // slices x stride x (8 d + 4) bytes and the index array, without overflow: stride < 2^33 and d <= 16, so a slice is below 2^41 bytes
  const size_t per_x = pf->stride * (size_t)pf->d * 8, per_a = pf->stride * 4, idx = (size_t)pf->n * 4;
  const size_t limit = ~(size_t)0 - idx - 64;
  if ((size_t)slices > limit / (per_x + per_a))
    return fail(CSSM_ENOMEM, "a window of %u slices of %zu bytes each does not fit (more than 2^64 bytes)", slices, per_x + per_a);
  const size_t bytes = (size_t)slices * (per_x + per_a) + idx;
  size_t free_b = 0, total_b = 0;
  HIP_TRY(hipMemGetInfo(&free_b, &total_b));
  if (bytes > total_b) return fail(CSSM_ENOMEM, "a window of %u slices does not fit (%zu bytes; the device has %zu)", slices, bytes, total_b);
  PfWindow* W = new PfWindow();
  pf->win = W;
  if (hipMalloc((void**)&W->X, (size_t)slices * per_x) != hipSuccess || hipMalloc((void**)&W->A, (size_t)slices * per_a) != hipSuccess ||
      hipMalloc((void**)&W->b, idx) != hipSuccess) {
    (void)hipGetLastError();
    window_free(pf);
    return fail(CSSM_ENOMEM, "a window of %u slices does not fit (%zu bytes)", slices, bytes);
  }
  if (hipEventCreate(&W->ev0) != hipSuccess || hipEventCreate(&W->ev1) != hipSuccess) { window_free(pf); return fail(CSSM_EHIP, "hipEventCreate for the window"); }
  W->time.assign(slices, 0.0);
  W->weighted.assign(slices, 0);
  cssm_window_open(&pf->wring, slices);
  return CSSM_OK;
}

extern "C" uint32_t cssm_pf_window_depth(const cssm_pf* pf) { return (pf && pf->win) ? cssm_window_depth(&pf->wring) : 0u; }

static void li_put(cssm_pf* pf, PfWindow* W, uint32_t slot, const double* src, size_t src_stride, const uint32_t* gather, const uint32_t* anc_src) {
  const size_t slab = pf->stride * (size_t)pf->d;
  hipLaunchKernelGGL(k_slice_put, dim3(grid_for(pf->n, 256, kGridCap)), dim3(256), 0, pf->stream, src, src_stride, gather, anc_src, (uint64_t)pf->n,
                     pf->d, W->X + (size_t)slot * slab, (size_t)pf->stride, W->A + (size_t)slot * pf->stride, (const Scalars*)pf->sc);
}

// Behind the step's launches (after a redo: again): the cloud the step proposed and the ancestors that resampled it into the newest slot,
// then row j = 0 .. nrows - 1 from slice (newest - j), each composing the lineage one slice further back; the end of the call's device
// time; the rows and their ticks on their way to the host.  No allocation, event or read-back between the rows.
int cssm_li_enqueue(cssm_pf* pf) {
  PfWindow* W = static_cast<PfWindow*>(pf->win);
  IvScratch* s = static_cast<IvScratch*>(pf->li);
  if (!W || pf->wring.count < 2u || (W->nrows && (!s || !s->keys || W->nrows > s->rows_cap)) || W->nrows > pf->wring.count)
    return fail(CSSM_ESTATE, "lineage rows outside the handle's window");
  const uint32_t newest = pf->wring.newest;
  W->weighted[newest] = pf->anc_valid ? 1 : 0;
  li_put(pf, W, newest, pf->src, pf->src_stride, nullptr, pf->anc_valid ? pf->anc : nullptr);
  if (W->nrows) {
    const int d = pf->d, rows = d + 1;
    const size_t slab = pf->stride * (size_t)d;
    const IvArgs a = iv_args(pf, s, rows);
    for (uint32_t j = 0; j < W->nrows; ++j) {
      const uint32_t slot = cssm_window_slot(&pf->wring, j);
      DISPATCH_D(d, k_lineage_fill<D><<<dim3(s->nblocks), dim3(CSSM_BLOCK), 0, pf->stream>>>(
                        W->X + (size_t)slot * slab, (size_t)pf->stride, W->weighted[slot] ? W->A + (size_t)slot * pf->stride : nullptr,
                        j ? W->b : nullptr, W->b, (uint64_t)pf->n, s->fco + (size_t)j * CSSM_MAX_DIM, pf->mk, s->keys, s->partial, s->pmm, s->zero,
                        s->zero_words, pf->sc, s->stamp));
      iv_launch_rounds(pf, a);
      hipLaunchKernelGGL(k_iv_finish, dim3(rows), dim3(CSSM_BLOCK), 0, pf->stream, a, s->rows + (size_t)j * s->out_stride, s->stamp);
    }
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(W->ev1, pf->stream));
  if (W->nrows) {
    HIP_TRY(hipMemcpyAsync(s->h_rows, s->rows, (size_t)W->nrows * s->out_stride * 8, hipMemcpyDeviceToHost, pf->stream));
    HIP_TRY(hipMemcpyAsync(s->h_rows + s->rows_cap * s->out_stride, s->stamp, 16, hipMemcpyDeviceToHost, pf->stream));
  }
  return CSSM_OK;
}

bool cssm_li_has_rows(const cssm_pf* pf) { return pf->win && static_cast<const PfWindow*>(pf->win)->nrows != 0u; }

extern "C" int cssm_pf_step_interpolate(cssm_pf* pf, double t, double obs, int has_obs, uint32_t lag, double interval, double* ll_out,
                                        int32_t* ess_out, uint32_t* rows_out, double* state_mean, double* state_lower, double* state_upper,
                                        double* eta_of_mean, double* eta_lower, double* eta_upper) {
  if (!pf) return fail(CSSM_EINVAL_ARG, "null handle");
  if (!(interval > 0.0 && interval <= 1.0)) return fail(CSSM_EINVAL_ARG, "interval must be in (0, 1]");
  int rc = li_refuse_handle(pf);
  if (rc) return rc;
  PfWindow* W = static_cast<PfWindow*>(pf->win);
  if (!W) return fail(CSSM_ESTATE, "the handle has no window: cssm_pf_window first");
  const bool want = lag != CSSM_PF_NO_ROWS;
  if (want && lag >= pf->wring.slices)
    return fail(CSSM_EINVAL_ARG, "a lag of %u reaches behind a window of %u slices (at most slices - 1)", lag, pf->wring.slices);
  if (!pf->initialised) return fail(CSSM_ESTATE, "cssm_pf_step before cssm_pf_init");
  HIP_TRY(hipSetDevice(pf->device));
  if (want) { rc = iv_ensure(pf, pf->li, false, (size_t)lag + 1, interval); if (rc) return rc; }   // (before the window moves: a refusal leaves it as it was)
  IvScratch* s = static_cast<IvScratch*>(pf->li);
  W->timed = false; W->ms0 = -1.0; W->ticks = 0ull;
  HIP_TRY(hipEventRecord(W->ev0, pf->stream));
  if (pf->wring.count == 0u) {   // a window that (re)starts: the cloud the handle holds now is its base slice, at the handle's clock
    const uint32_t slot = cssm_window_put(&pf->wring);
    W->time[slot] = pf->t; W->weighted[slot] = 0;
    li_put(pf, W, slot, pf->src, pf->src_stride, pf->anc_valid ? pf->anc : nullptr, nullptr);
  }
  const uint32_t slot = cssm_window_put(&pf->wring);
  W->time[slot] = t;
  W->nrows = want ? cssm_window_rows(&pf->wring, lag) : 0u;
  if (want) {   // the f coefficients of every row: F(t) of its slice's time, as cssm_pf_summary builds them -- one upload
    s->h_fco.assign((size_t)W->nrows * CSSM_MAX_DIM, 0.0);
    StepRec hrec;
    for (uint32_t j = 0; j < W->nrows; ++j) {
      const double time = W->time[cssm_window_slot(&pf->wring, j)];
      cssm_build_rec(pf, time, time, 0.0, 0, pf->step, &hrec);
      memcpy(&s->h_fco[(size_t)j * CSSM_MAX_DIM], hrec.fco, sizeof hrec.fco);
    }
    rc = hipMemcpyAsync(s->fco, s->h_fco.data(), s->h_fco.size() * 8, hipMemcpyHostToDevice, pf->stream) == hipSuccess &&
                 hipMemsetAsync(s->stamp, 0, 16, pf->stream) == hipSuccess
             ? CSSM_OK
             : fail(CSSM_EHIP, "the f coefficients of the lineage rows");
  }
  if (!rc) rc = cssm_step_rows(pf, t, obs, has_obs, ll_out, ess_out, CSSM_ROWS_LINEAGE);
  if (rc) { cssm_window_restart(&pf->wring); return rc; }   // (a failed step leaves no slice to build on)
  if (want) {
    iv_unpack(pf, s, W->nrows, state_mean, state_lower, state_upper, eta_of_mean, eta_lower, eta_upper);
    memcpy(&W->ticks, reinterpret_cast<const char*>(s->h_rows + s->rows_cap * s->out_stride) + 8, 8);
    const int d = pf->d;
    for (size_t r = W->nrows; r <= (size_t)lag; ++r) {   // rows the window does not reach
      for (int k = 0; k < d; ++k) {
        if (state_mean) state_mean[r * d + k] = cssm_nan();
        if (state_lower) state_lower[r * d + k] = cssm_nan();
        if (state_upper) state_upper[r * d + k] = cssm_nan();
      }
      if (eta_of_mean) eta_of_mean[r] = cssm_nan();
      if (eta_lower) eta_lower[r] = cssm_nan();
      if (eta_upper) eta_upper[r] = cssm_nan();
    }
  }
  if (rows_out) *rows_out = W->nrows;
  W->timed = true;
  return CSSM_OK;
}

extern "C" int cssm_pf_step_interpolate_last_ms(cssm_pf* pf, double* ms2) {
  if (!pf || !ms2) return fail(CSSM_EINVAL_ARG, "null argument");
  PfWindow* W = static_cast<PfWindow*>(pf->win);
  if (!W || !W->timed) return fail(CSSM_ESTATE, "no call of cssm_pf_step_interpolate has completed on this handle's window");
  if (W->ms0 < 0.0) {
    HIP_TRY(hipSetDevice(pf->device));
    float ms = 0.f;
    HIP_TRY(hipEventSynchronize(W->ev1));
    HIP_TRY(hipEventElapsedTime(&ms, W->ev0, W->ev1));
    W->ms0 = (double)ms;
  }
  ms2[0] = W->ms0;
  ms2[1] = W->nrows ? (double)W->ticks * 1e-5 : 0.0;   // 100 MHz
  return CSSM_OK;
}
