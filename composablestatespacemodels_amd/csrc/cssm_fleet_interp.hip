// cssm_fleet_interp.hip -- the backward pass of cssm_fleet_interpolate (include/cssm_pf.h): the lineages that survive to the end of
// every series, summarised per time index (FilterInterpolate, model/ParticleFilter.scala:273-311; examples/Interpolate.scala:42-44),
// in ONE launch for a chunk of series.  The forward pass (k_fleet_series<D, false, true>, cssm_fleet.hip.h) left every cloud X_s and,
// behind every weighted record, the ancestors anc_s that resampled it; the state at time index s of final path i is X_s[b_s(i)] with
// b_T = anc_T (the identity behind an unweighted record) and b_{s-1} = anc_{s-1}[b_s] -- cssm_pf_interpolate's k_compose, T launches
// there, a loop in LDS here.
//
// One block per (series, row), 256 threads.  Each of the d + 1 blocks of a series composes b itself (N loads of ancestors per time
// index), so no block reads what another one wrote: no atomics on global memory, no flag, every loop bounded by N or by T_k.  A
// thread owns the same slots i = tid, tid + 256, ... of b in every phase, so the composition and the gather need no barrier of their
// own.  The row summary is k_fleet_summary's statement: the values as order-preserving keys, a bitonic network over the next power
// of two in LDS (padded with the largest key), the mean a plain fp64 sum.  It is stated here a third time (k_fleet_summary,
// fleet_forecast_body): one __device__ function for the three is held back until the resource report of the two existing kernels can
// be compared with it in place.
//
// Dynamic LDS: np2 keys (8 bytes each) + N uint32 of b -- 48 KiB at N = 4096, three blocks per CU.
#include <hip/hip_runtime.h>

#include "cssm_internal.h"
#include "cssm_kernels.hip.h"
#include "cssm_fleet_interp.hip.h"

template <int D>
__global__ __launch_bounds__(CSSM_BLOCK) void k_fleet_lineage(const FleetLinArgs a) {
  extern __shared__ unsigned long long s_keys[];
  __shared__ double s_p[CSSM_BLOCK / 64];
  const uint32_t n = a.n, np2 = a.np2, k = blockIdx.x, row = blockIdx.y, tid = threadIdx.x;
  uint32_t* s_b = reinterpret_cast<uint32_t*>(s_keys + np2);
  const unsigned long long r0 = a.off[k], r1 = a.off[k + 1];
  const uint32_t T = (uint32_t)(r1 - r0);
  const size_t base = (size_t)r0 + k;                           // the series' first slice and first output row
  if (T == 0u || a.ser[k].err != 0u) {                          // (uniform) no records, or unusable weights: every row reads NaN
    for (uint32_t o = 0; o <= T; ++o)
      if (tid < 3u) a.out[((base + o) * (D + 1) + row) * 3u + tid] = cssm_nan();
    return;
  }
  constexpr uint32_t RB = (uint32_t)CSSM_FLEET_REC_BYTES(D);
  for (uint32_t i = tid; i < n; i += CSSM_BLOCK) s_b[i] = i;
  for (uint32_t s = T + 1u; s-- > 0u;) {                        // bounded by the series' length
    __syncthreads();                                            // the row sorted last is read; s_p is free
    const bool resampled = s >= 1u && reinterpret_cast<const FleetRecHead*>(a.recs + ((size_t)r0 + s - 1u) * RB)->has_obs != 0;
    const uint32_t* ga = a.hanc + (base + s) * n;
    const double* src = a.hist + (base + s) * D * n;
    const uint32_t o = a.pairing ? T - s : s;
    const double* fco = a.fco + (base + o) * D;
    double acc = 0.0;
    for (uint32_t i = tid; i < np2; i += CSSM_BLOCK) {
      unsigned long long key = ~0ull;
      if (i < n) {
        uint32_t j = s_b[i];
        if (resampled) { j = ga[j]; s_b[i] = j; }
        double v;
        if (row < (uint32_t)D) {
          v = src[(size_t)row * n + j];
        } else {
          double x[D];
#pragma unroll
          for (int q = 0; q < D; ++q) x[q] = src[(size_t)q * n + j];
          v = link_of(a.mk.obs_kind, gamma_coef<D>(a.mk, fco, x));
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
      double* out = a.out + ((base + o) * (D + 1) + row) * 3u;
      out[0] = sum / (double)n;
      out[1] = cssm_order_unkey(s_keys[row < (uint32_t)D ? a.lo_state : a.lo_eta]);
      out[2] = cssm_order_unkey(s_keys[row < (uint32_t)D ? a.hi_state : a.hi_eta]);
    }
  }
}

int cssm_fleet_lineage_launch(const FleetLinLaunch& l) {
  const size_t lds = (size_t)l.args.np2 * 8u + (size_t)l.args.n * 4u;
  DISPATCH_D(l.d, hipLaunchKernelGGL(k_fleet_lineage<D>, dim3(l.n_series, D + 1), dim3(CSSM_BLOCK), lds, l.stream, l.args));
  return (int)hipGetLastError();
}
