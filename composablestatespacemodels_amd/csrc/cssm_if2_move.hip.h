// cssm_if2_move.hip.h -- the two device statements of the contract's iterated filtering (include/cssm_numerics.h, "iterated filtering")
// that both of its kernels' files make: k_fleet_if2 (cssm_fleet_if2.hip, a swarm per workgroup) and the launches of cssm_pf_if2
// (cssm_if2.hip, one swarm tiled over many workgroups).
#pragma once

#include "cssm_fleet.hip.h"

// theta[.][i] of the destination = theta[.][a] of the source, perturbed where sd[j] != 0 (`sd`: LDS, padded with zeros to a multiple
// of four).  One Philox block serves four slots: normal j of the stream is element j & 1 of pair j >> 1 (cssm_if2_normal).
__device__ __forceinline__ void if2_move(const double* __restrict__ src, uint32_t a, double* __restrict__ dst, uint32_t i, uint32_t n, uint32_t nt,
                                         uint64_t key, uint32_t when, const double* sd, const double* tab) {
  for (uint32_t j0 = 0; j0 < nt; j0 += 4u) {
    const double s[4] = {sd[j0], sd[j0 + 1u], sd[j0 + 2u], sd[j0 + 3u]};
    double e[4] = {0.0, 0.0, 0.0, 0.0};
    const bool p0 = s[0] != 0.0 || s[1] != 0.0, p1 = s[2] != 0.0 || s[3] != 0.0;   // (uniform)
    if (p0 || p1) {
      const cssm_u32x4 blk = cssm_philox_draw(key, (uint64_t)i, when, CSSM_STREAM_IF2, j0 >> 2);
      if (p0) cssm_normal_pair64(blk.v[0], blk.v[1], tab, &e[0], &e[1]);
      if (p1) cssm_normal_pair64(blk.v[2], blk.v[3], tab, &e[2], &e[3]);
    }
#pragma unroll
    for (uint32_t q = 0; q < 4u; ++q) {
      const uint32_t j = j0 + q;
      if (j < nt) {
        double th = src[(size_t)j * n + a];
        if (s[q] != 0.0) th = cssm_if2_perturb(th, s[q], e[q]);
        dst[(size_t)j * n + i] = th;
      }
    }
  }
}

// a component's constrained field from the particle's own row (0.0 where its SDE has no such field, as the descriptor path leaves it)
__device__ __forceinline__ double if2_field(const If2Map& map, int kind, int c, int field, const double* th, uint32_t i, uint32_t n) {
  const int slot = map.slot[c][field];
  return slot < 0 ? 0.0 : cssm_constrain(kind, field, th[(size_t)slot * n + i]);
}
