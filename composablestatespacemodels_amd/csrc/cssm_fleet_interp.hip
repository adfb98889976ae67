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
// own.  cssm_fleet_step_interpolate's k_fleet_window walks the slots of a series' window with the same body (fleet_lineage_body: the two
// differ in where their slices lie).  The row summary is k_fleet_summary's statement: the values as order-preserving keys, a bitonic network over the next power
// of two in LDS (padded with the largest key), the mean a plain fp64 sum.  It is stated here a third time (k_fleet_summary,
// fleet_forecast_body): one __device__ function for the three is held back until the resource report of the two existing kernels can
// be compared with it in place.
//
// Dynamic LDS: np2 keys (8 bytes each) + N uint32 of b -- 48 KiB at N = 4096, three blocks per CU.
#include <hip/hip_runtime.h>

#include "cssm_internal.h"
#include "cssm_kernels.hip.h"
#include "cssm_fleet_interp.hip.h"
#include "cssm_fleet_rows.hip.h"

// Where the slices a block walks lie -- newest first -- and where each one's row goes: the whole history of a series
// (cssm_fleet_interpolate) or the window of one (cssm_fleet_step_interpolate).  Step j of `steps`: cloud(j) / anc(j) the slice,
// resampled(j) whether its ancestors exist (the slice was written by a weighted record), fco(j) F at its time, out(j) its [d + 1][3].
template <int D>
struct FleetLinHist {                                           // slices base .. base + T of hist / hanc, output row o = s or T - s
  static constexpr bool kDirect = false;
  const FleetLinArgs& a;
  size_t base; unsigned long long r0; uint32_t T;
  __device__ __forceinline__ uint32_t slice(uint32_t j) const { return T - j; }
  __device__ __forceinline__ uint32_t row(uint32_t j) const { return a.pairing ? j : T - j; }
  __device__ __forceinline__ bool resampled(uint32_t j) const {
    const uint32_t s = slice(j);
    return s >= 1u && reinterpret_cast<const FleetRecHead*>(a.recs + ((size_t)r0 + s - 1u) * (uint32_t)CSSM_FLEET_REC_BYTES(D))->has_obs != 0;
  }
  __device__ __forceinline__ const uint32_t* anc(uint32_t j) const { return a.hanc + (base + slice(j)) * a.n; }
  __device__ __forceinline__ const double* cloud(uint32_t j) const { return a.hist + (base + slice(j)) * D * a.n; }
  __device__ __forceinline__ const double* fco(uint32_t j) const { return a.fco + (base + row(j)) * D; }
  __device__ __forceinline__ double* out(uint32_t j) const { return a.out + (base + row(j)) * (D + 1) * 3u; }
};
template <int D>
struct FleetLinWindow {                                         // request q: the slots words[j] of series k's window, output row q L + j
  static constexpr bool kDirect = false;
  const FleetWinArgs& a;
  uint32_t k, q;
  __device__ __forceinline__ uint32_t word(uint32_t j) const { return a.words[(size_t)q * a.L + j]; }
  __device__ __forceinline__ size_t slot(uint32_t j) const { return (size_t)k * a.slices + (word(j) & ~CSSM_FLEET_WIN_RESAMPLED); }
  __device__ __forceinline__ bool resampled(uint32_t j) const { return (word(j) & CSSM_FLEET_WIN_RESAMPLED) != 0u; }
  __device__ __forceinline__ const uint32_t* anc(uint32_t j) const { return a.ring_a + slot(j) * a.n; }
  __device__ __forceinline__ const double* cloud(uint32_t j) const { return a.ring_x + slot(j) * D * a.n; }
  __device__ __forceinline__ const double* fco(uint32_t j) const { return a.fco + ((size_t)q * a.L + j) * D; }
  __device__ __forceinline__ double* out(uint32_t j) const { return a.out + ((size_t)q * a.L + j) * (D + 1) * 3u; }
};

// (the walk itself -- fleet_lineage_body -- is cssm_fleet_rows.hip.h: the backward-simulation summaries of cssm_fleet_smooth.hip share it)
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
  fleet_lineage_body<D>(FleetLinHist<D>{a, base, r0, T}, T + 1u, n, np2, row, a.mk, a.lo_state, a.hi_state, a.lo_eta, a.hi_eta, s_keys, s_b, s_p);
}

// cssm_fleet_step_interpolate's second launch: one block per (series that asked for rows, row), over the slots of the series' window
// the host named, newest first.  A series the forward launch gave up leaves its rows as they were preset (NaN).
template <int D>
__global__ __launch_bounds__(CSSM_BLOCK) void k_fleet_window(const FleetWinArgs a) {
  extern __shared__ unsigned long long s_keys[];
  __shared__ double s_p[CSSM_BLOCK / 64];
  const uint32_t q = blockIdx.x, row = blockIdx.y;
  const FleetWinReq rq = a.req[q];
  if (a.ser[rq.k].err != 0u) return;                            // (uniform)
  uint32_t* s_b = reinterpret_cast<uint32_t*>(s_keys + a.np2);
  fleet_lineage_body<D>(FleetLinWindow<D>{a, rq.k, q}, rq.rows, a.n, a.np2, row, a.mk, a.lo_state, a.hi_state, a.lo_eta, a.hi_eta, s_keys, s_b, s_p);
}

int cssm_fleet_lineage_launch(const FleetLinLaunch& l) {
  const size_t lds = (size_t)l.args.np2 * 8u + (size_t)l.args.n * 4u;
  DISPATCH_D(l.d, hipLaunchKernelGGL(k_fleet_lineage<D>, dim3(l.n_series, D + 1), dim3(CSSM_BLOCK), lds, l.stream, l.args));
  return (int)hipGetLastError();
}

int cssm_fleet_window_launch(const FleetWinLaunch& l) {
  const size_t lds = (size_t)l.args.np2 * 8u + (size_t)l.args.n * 4u;
  DISPATCH_D(l.d, hipLaunchKernelGGL(k_fleet_window<D>, dim3(l.n_req, D + 1), dim3(CSSM_BLOCK), lds, l.stream, l.args));
  return (int)hipGetLastError();
}
