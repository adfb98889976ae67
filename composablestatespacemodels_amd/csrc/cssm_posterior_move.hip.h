// cssm_posterior_move.hip.h -- what moves a particle of a posterior-predictive forecast, shared by the single handle's kernel
// (cssm_forecast.hip: k_forecast_post) and the fleet's (cssm_fleet_forecast.hip: k_fleet_forecast_post): the pair loop over the
// CSSM_STREAM_STEP normals, a particle's own parameter set, and the one statement that moves a component under it.  One text, so the
// two kernels give equal bits by construction.
#pragma once

#include "cssm_device.hip.h"
#include "cssm_sde_coef.h"

// The 2 D normals of the pair (2m, 2m+1) as propagate_pair (cssm_device.hip.h) draws them: its ceil(D / 2) Philox blocks in order, each
// normal handed to feed(b, k, e) as soon as it exists -- normal q goes to particle b = q / D of the pair, component k = q % D.  Every
// forecast source that steps whole pairs outside propagate_pair goes through this loop.  MUST CHANGE TOGETHER WITH propagate_pair, which
// keeps its own statement of the loop: k_propagate's code changes when its loop goes through a callable
// (profiles/forecast_body_pair_loop_asm.md), and that kernel is not to move.  tests/test_gpu_forecast.py holds k_forecast to the
// oracle's propagate bit for bit.
template <int D, class Feed>
__device__ __forceinline__ void pair_normals_feed(uint64_t seed, uint64_t gid_even, uint32_t step, const double* tab, Feed&& feed) {
  const uint64_t stream = cssm_pair_stream(gid_even);
  auto give = [&](int q, double e) {            // (q is a compile-time constant wherever this is called)
    if (q < 2 * D) feed(q / D, q % D, e);
  };
#pragma unroll
  for (int B = 0; B < (D + 1) / 2; ++B) {
    const cssm_u32x4 blk = cssm_philox_draw(seed, stream, step, CSSM_STREAM_STEP, (uint32_t)B);
    double e0, e1;
    cssm_normal_pair64(blk.v[0], blk.v[1], tab, &e0, &e1);
    give(4 * B, e0); give(4 * B + 1, e1);
    if (2 * B + 1 < D) {
      cssm_normal_pair64(blk.v[2], blk.v[3], tab, &e0, &e1);
      give(4 * B + 2, e0); give(4 * B + 3, e1);
    }
  }
}

// A particle's parameter set: the 3 D constrained values (mu, phi, sigma) of its posterior row (cssm_posterior_rows), held in
// registers (REG) or read from the row where two particles' sets would spill (the row is L2-resident: 3 D + 1 doubles per pair of the
// sample).  The single handle keeps them in registers up to D = 8; the fleet's kernel names its own threshold.
template <int D, bool REG = (D <= 8)>
struct PostParams {
  double v[3 * D];
  __device__ __forceinline__ void load(const double* __restrict__ row) {
#pragma unroll
    for (int k = 0; k < 3 * D; ++k) v[k] = row[k];
  }
  __device__ __forceinline__ double mu(int k) const { return v[3 * k]; }
  __device__ __forceinline__ double phi(int k) const { return v[3 * k + 1]; }
  __device__ __forceinline__ double sigma(int k) const { return v[3 * k + 2]; }
};
template <int D>
struct PostParams<D, false> {
  const double* row;
  __device__ __forceinline__ void load(const double* __restrict__ r) { row = r; }
  __device__ __forceinline__ double mu(int k) const { return row[3 * k]; }
  __device__ __forceinline__ double phi(int k) const { return row[3 * k + 1]; }
  __device__ __forceinline__ double sigma(int k) const { return row[3 * k + 2]; }
};

// One component under the particle's own parameters: transition_step on the coefficients cssm_sde_coef gives for them (what
// cssm_build_rec puts into a record for a model's parameters): the same arithmetic, so equal parameters give equal bits.
template <class Params>
__device__ __forceinline__ void post_move(int kind, const Params& prm, int k, double dt, double& xk, double zk) {
  double c[4];
  cssm_sde_coef(kind, prm.mu(k), prm.phi(k), prm.sigma(k), dt, c);
  transition_step(kind, c[0], c[1], c[2], c[3], dt, xk, zk);
}

// One transition of the pair (ia, ia + 1) at step h under the parameter sets pa / pb, or of particle ia alone (the unpaired last
// particle of an odd cloud, keyed as propagate_one keys it).
template <int D, class Params>
__device__ __forceinline__ void post_step(bool hasb, const ModelK& mk, double dt, uint64_t key, uint64_t ia, uint32_t h, const double* tab,
                                          const Params& pa, const Params& pb, double (&xa)[D], double (&xb)[D]) {
  if (hasb) {
    pair_normals_feed<D>(key, ia, h, tab, [&](int b, int k, double e) { post_move(mk.kind(k), b ? pb : pa, k, dt, b ? xb[k] : xa[k], e); });
  } else {
    double z[D];
    draw_normals<D>(key, ia, h, CSSM_STREAM_STEP, tab, z);
#pragma unroll
    for (int k = 0; k < D; ++k) post_move(mk.kind(k), pa, k, dt, xa[k], z[k]);
  }
}
