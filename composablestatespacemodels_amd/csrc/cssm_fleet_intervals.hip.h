// cssm_fleet_intervals.hip.h -- getIntervals (model/ParticleFilter.scala:415-424) of ONE cloud by the workgroup that holds it: the d + 1
// row summaries k_fleet_series<D, false, false, true> writes behind the initial draw and behind every record (cssm_fleet_filter_intervals,
// cssm_fleet_step_intervals).  Rows 0 .. D-1 are the state components, row D eta = link(f(x, t)); per row the mean (a plain fp64 sum / N)
// and the two order statistics at sel_ranks' ranks, exact: the row's N values are sorted in LDS as order-preserving keys (bitonic network
// over the next power of two, padded with the largest key) -- k_fleet_summary's statement, run by a block of any size once per row.
#pragma once

#include "cssm_device.hip.h"

// the ranks of a state row and of the eta row, as the host takes them from sel_ranks
struct FleetRowRanks {
  uint32_t lo_state, hi_state, lo_eta, hi_eta;
};

// What the row summaries of a forecast share (fleet_forecast_body of cssm_fleet_forecast.hip, fleet_onestep_forecast of
// cssm_fleet_onestep.hip.h), written once.  fleet_cloud_intervals below keeps its own statement of the network: it adds a row in another
// order (k_fleet_summary's), and called from there the shared function moved the registers of k_fleet_series<6, false, false, true>
// (211 -> 168 VGPRs), which no change to another instantiation may do.
// fleet_sort_keys: k_fleet_summary's bitonic network over the np2 keys of a row in LDS, ascending; every stage opens with a barrier (so
// the keys may have been written just before the call), the caller closes with one before it reads a rank.
__device__ __forceinline__ void fleet_sort_keys(unsigned long long* s_keys, uint32_t np2, uint32_t tid, uint32_t bs) {
  for (uint32_t k2 = 2u; k2 <= np2; k2 <<= 1) {
    for (uint32_t j = k2 >> 1; j > 0u; j >>= 1) {
      __syncthreads();
      for (uint32_t i = tid; i < np2; i += bs) {
        const uint32_t p = i ^ j;
        if (p > i) {
          const unsigned long long x = s_keys[i], y = s_keys[p];
          const bool up = (i & k2) == 0u;
          if ((x > y) == up) { s_keys[i] = y; s_keys[p] = x; }
        }
      }
    }
  }
}
// fleet_row_keys: the n values of a row (`v`, written by this block behind a barrier) as order-preserving keys, padded to np2 with the
// largest key, and the row's sum in a forecast's order of additions -- thread tid adds v[tid], v[tid + blockDim], ..., a butterfly over
// each wave, the waves' sums in s_p for the thread that adds them left to right.  Both forecasts of a fleet run blocks of the fleet's
// one size, so a row's mean has the same bits from either.
__device__ __forceinline__ void fleet_row_keys(const double* v, uint32_t n, uint32_t np2, unsigned long long* s_keys, double* s_p) {
  const uint32_t tid = threadIdx.x, bs = blockDim.x;
  double acc = 0.0;
  for (uint32_t i = tid; i < np2; i += bs) {
    unsigned long long kk = ~0ull;
    if (i < n) { const double x = v[i]; acc += x; kk = cssm_order_key(x); }
    s_keys[i] = kk;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
  if ((tid & 63u) == 0u) s_p[tid >> 6] = acc;
}

// The cloud is `buf` ([D][n], SoA) read through `s_anc` (LDS, n entries); `s_keys` holds np2 keys of LDS nothing else uses meanwhile,
// np2 the power of two >= max(n, 2); `fco` the D f coefficients at the cloud's time (any address space); `out` = [D + 1][3]: mean, lower,
// upper.  Every thread of the block calls it, behind a barrier that completed buf and s_anc; it ends behind a barrier of its own, so
// s_keys is free again on return.  log2(np2) (log2(np2) + 1) / 2 + 3 barriers per row; every loop is bounded by np2, CSSM_BLOCK or D.
template <int D>
__device__ __forceinline__ void fleet_cloud_intervals(const double* buf, const uint32_t* s_anc, uint32_t n, uint32_t np2, const ModelK& mk,
                                                      const double* fco, const FleetRowRanks& rk, unsigned long long* s_keys, double* out) {
  __shared__ double s_p[CSSM_BLOCK / 64];
  const uint32_t tid = threadIdx.x, bs = blockDim.x;
  for (uint32_t row = 0; row <= (uint32_t)D; ++row) {
    for (uint32_t i = tid; i < np2; i += bs) {
      unsigned long long key = ~0ull;
      if (i < n) {
        const uint32_t j = s_anc[i];
        double v;
        if (row < (uint32_t)D) {
          v = buf[(size_t)row * n + j];
        } else {
          double x[D];
#pragma unroll
          for (int q = 0; q < D; ++q) x[q] = buf[(size_t)q * n + j];
          v = link_of(mk.obs_kind, gamma_coef<D>(mk, fco, x));
        }
        key = cssm_order_key(v);
      }
      s_keys[i] = key;
    }
    __syncthreads();
    // the mean in k_fleet_summary's order of additions whatever the block's size is: CSSM_BLOCK partial sums of stride CSSM_BLOCK, a
    // butterfly over each wave of them, the waves' sums left to right -- so a row's mean has the bits cssm_fleet_summary gives it.  The
    // block's threads stand in for the CSSM_BLOCK: thread tid takes tid, tid + bs, ... below CSSM_BLOCK (whole waves: bs is a multiple of 64).
    for (uint32_t v = tid; v < (uint32_t)CSSM_BLOCK; v += bs) {   // (wave-uniform trip count)
      double acc = 0.0;
      for (uint32_t i = v; i < n; i += CSSM_BLOCK) acc += cssm_order_unkey(s_keys[i]);
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
      if ((v & 63u) == 0u) s_p[v >> 6] = acc;
    }
    for (uint32_t k2 = 2u; k2 <= np2; k2 <<= 1) {
      for (uint32_t j = k2 >> 1; j > 0u; j >>= 1) {
        __syncthreads();
        for (uint32_t i = tid; i < np2; i += bs) {
          const uint32_t p = i ^ j;
          if (p > i) {
            const unsigned long long x = s_keys[i], y = s_keys[p];
            const bool up = (i & k2) == 0u;
            if ((x > y) == up) { s_keys[i] = y; s_keys[p] = x; }
          }
        }
      }
    }
    __syncthreads();
    if (tid == 0) {
      double s = 0.0;
      for (int w = 0; w < CSSM_BLOCK / 64; ++w) s += s_p[w];
      double* o = out + (size_t)row * 3u;
      o[0] = s / (double)n;
      o[1] = cssm_order_unkey(s_keys[row < (uint32_t)D ? rk.lo_state : rk.lo_eta]);
      o[2] = cssm_order_unkey(s_keys[row < (uint32_t)D ? rk.hi_state : rk.hi_eta]);
    }
    __syncthreads();                                            // the keys and the waves' partial sums are free for the next row
  }
}
