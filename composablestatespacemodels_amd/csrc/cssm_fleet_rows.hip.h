// cssm_fleet_rows.hip.h -- the row summaries of a walk over the slices of a series, newest first: the body k_fleet_lineage, k_fleet_window
// (cssm_fleet_interp.hip) and k_fleet_smooth_rows (cssm_fleet_smooth.hip) share.  A source type says where the slices lie, where each
// one's row goes and -- Src::kDirect -- how slot i of a slice is reached:
//   false  through the lineages that survive to the newest slice: b = the identity; per slice b = anc[b] where the slice resampled;
//   true   through an index array of the slice's own (anc(j)[i] IS the particle: the backward-simulated trajectories), n of them over a
//          cloud whose rows are ld() apart.
#pragma once

#include "cssm_fleet.hip.h"

// Row `row` of every slice's cloud through its indices -- keys, bitonic sort over np2, the mean (slots tid + 256 q per thread, the
// xor-shuffle tree, the wave partials added in wave order).
template <int D, class Src>
__device__ __forceinline__ void fleet_lineage_body(const Src& src_of, uint32_t steps, uint32_t n, uint32_t np2, uint32_t row, const ModelK& mk,
                                                   uint32_t lo_state, uint32_t hi_state, uint32_t lo_eta, uint32_t hi_eta,
                                                   unsigned long long* s_keys, uint32_t* s_b, double* s_p) {
  const uint32_t tid = threadIdx.x;
  uint32_t ld = n;                                              // the distance between the rows of a cloud
  if constexpr (Src::kDirect) ld = src_of.ld();
  else
    for (uint32_t i = tid; i < n; i += CSSM_BLOCK) s_b[i] = i;
  for (uint32_t st = 0; st < steps; ++st) {                     // bounded by the series' length / the window's
    __syncthreads();                                            // the row sorted last is read; s_p is free
    const bool resampled = src_of.resampled(st);
    const uint32_t* ga = src_of.anc(st);
    const double* src = src_of.cloud(st);
    const double* fco = src_of.fco(st);
    double acc = 0.0;
    for (uint32_t i = tid; i < np2; i += CSSM_BLOCK) {
      unsigned long long key = ~0ull;
      if (i < n) {
        uint32_t j;
        if constexpr (Src::kDirect) {
          j = ga[i];
        } else {
          j = s_b[i];
          if (resampled) { j = ga[j]; s_b[i] = j; }
        }
        double v;
        if (row < (uint32_t)D) {
          v = src[(size_t)row * ld + j];
        } else {
          double x[D];
#pragma unroll
          for (int q = 0; q < D; ++q) x[q] = src[(size_t)q * ld + j];
          v = link_of(mk.obs_kind, gamma_coef<D>(mk, fco, x));
        }
        acc += v;
        key = cssm_order_key(v);
      }
      s_keys[i] = key;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
    if ((tid & 63u) == 0u) s_p[tid >> 6] = acc;
    for (uint32_t k2 = 2u; k2 <= np2; k2 <<= 1) {
      for (uint32_t j = k2 >> 1; j > 0u; j >>= 1) {
        __syncthreads();
        for (uint32_t i = tid; i < np2; i += CSSM_BLOCK) {
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
      double sum = 0.0;
      for (int w = 0; w < CSSM_BLOCK / 64; ++w) sum += s_p[w];
      double* out = src_of.out(st) + (size_t)row * 3u;
      out[0] = sum / (double)n;
      out[1] = cssm_order_unkey(s_keys[row < (uint32_t)D ? lo_state : lo_eta]);
      out[2] = cssm_order_unkey(s_keys[row < (uint32_t)D ? hi_state : hi_eta]);
    }
  }
}
