// cssm_fleet_copy.hip.h -- k_fleet_copy, the gather over series behind cssm_fleet_copy_series (cssm_fleet.hip launches it): whole series
// -- cloud, ancestors, scalars -- move between the series of one fleet or from a second fleet of the same shape.  EXTENSION: the
// reference has no operation that writes one filter's cloud from another's.
//
// Blocks: (move, tile).  A move is one destination series the host decided to serve (kept, self-mapped and dead-source series get no
// block); its cloud is ONE contiguous run of d n doubles (the half of state[S][2][d][n] its observation index selects), its ancestors one
// run of n uint32, its scalars one FleetSeries.  Tile t of a move copies CSSM_FLEET_COPY_TILE doubles of the cloud, the t-th slice of the
// ancestors and (t = 0) the scalars.  Nothing waits on another block: what makes a simultaneous assignment of one fleet onto itself safe
// is the staging of the host (two launches; cssm_fleet_copy_series), not an order among blocks.
//
// Alignment: a cloud starts (2 k + half) d n doubles behind a 256-byte aligned allocation, so both ends are 16-byte aligned when both
// offsets are even -- always when d n is even; then the tile moves as double2 (16-byte loads and stores).  Otherwise it moves as doubles.
// In a whole tile a thread issues all its loads before its first store (named values, not an indexed array: the compiler moves such an
// array into LDS); the last, partial tile of a cloud is a plain strided loop.  No LDS, no scratch.
#pragma once

#include "cssm_fleet.hip.h"

#define CSSM_FLEET_COPY_THREADS 256
#define CSSM_FLEET_COPY_TILE 2048u      /* doubles of a cloud per block: 4 x 16 bytes (or 8 x 8 bytes) per thread */
#define CSSM_FLEET_COPY_CLOUD 1u        /* FleetCopyMove::flags: the move has a cloud to copy (a settling launch may only bring ancestors and scalars home) */

struct FleetCopyMove {
  unsigned long long src_x, dst_x;   // where the cloud starts in src_state / dst_state, in doubles
  uint32_t src_k, dst_k;             // the rows of src_anc / src_ser and of dst_anc / dst_ser
  uint32_t flags, pad_;
};
static_assert(sizeof(FleetCopyMove) == 32, "the table of a launch is staged as it is");
static_assert((unsigned long long)CSSM_MAX_DIM * CSSM_FLEET_MAX_N <= 0xffffffffull, "FleetCopyArgs::dn, d n of one cloud, is a uint32");

struct FleetCopyArgs {
  const FleetCopyMove* moves;        // [moves of the launch]
  const double* src_state;           // (the two may be one allocation: the regions a launch reads and writes are disjoint by the host's staging)
  double* dst_state;
  const uint32_t* src_anc;           // [.][n]
  uint32_t* dst_anc;
  const FleetSeries* src_ser;
  FleetSeries* dst_ser;
  uint32_t dn, n, tiles;             // d n; particles; tiles per move = ceil(dn / CSSM_FLEET_COPY_TILE)
};

__global__ __launch_bounds__(CSSM_FLEET_COPY_THREADS) void k_fleet_copy(FleetCopyArgs a) {
  const uint32_t m = blockIdx.x / a.tiles, tile = blockIdx.x - m * a.tiles, tid = threadIdx.x;
  constexpr uint32_t T = CSSM_FLEET_COPY_THREADS;
  const FleetCopyMove mv = a.moves[m];
  if (mv.flags & CSSM_FLEET_COPY_CLOUD) {   // (uniform)
    const uint32_t lo = tile * CSSM_FLEET_COPY_TILE, hi = min(a.dn, lo + CSSM_FLEET_COPY_TILE);
    const double* s = a.src_state + mv.src_x;
    double* d = a.dst_state + mv.dst_x;
    if (((mv.src_x | mv.dst_x) & 1ull) == 0ull) {   // (uniform) both ends 16-byte aligned; lo is even
      const double2* s2 = reinterpret_cast<const double2*>(s + lo);
      double2* d2 = reinterpret_cast<double2*>(d + lo);
      const uint32_t pairs = (hi - lo) >> 1;
      if (pairs == CSSM_FLEET_COPY_TILE / 2u) {   // (uniform) a whole tile: four loads in flight per thread, then four stores
        const double2 v0 = s2[tid], v1 = s2[tid + T], v2 = s2[tid + 2u * T], v3 = s2[tid + 3u * T];
        d2[tid] = v0; d2[tid + T] = v1; d2[tid + 2u * T] = v2; d2[tid + 3u * T] = v3;
      } else {
        for (uint32_t i = tid; i < pairs; i += T) d2[i] = s2[i];
        if (((hi - lo) & 1u) && tid == 0u) d[hi - 1u] = s[hi - 1u];   // (d n odd under two even offsets: the last tile's last double)
      }
    } else if (hi - lo == CSSM_FLEET_COPY_TILE) {   // (uniform) a whole tile, 8 bytes at a time
      const double* sp = s + lo + tid;
      double* dp = d + lo + tid;
      const double v0 = sp[0], v1 = sp[T], v2 = sp[2u * T], v3 = sp[3u * T], v4 = sp[4u * T], v5 = sp[5u * T], v6 = sp[6u * T], v7 = sp[7u * T];
      dp[0] = v0; dp[T] = v1; dp[2u * T] = v2; dp[3u * T] = v3; dp[4u * T] = v4; dp[5u * T] = v5; dp[6u * T] = v6; dp[7u * T] = v7;
    } else {
      for (uint32_t i = lo + tid; i < hi; i += T) d[i] = s[i];
    }
  }
  {   // the tile's slice of the ancestors
    const uint32_t per = (a.n + a.tiles - 1u) / a.tiles, lo = min(a.n, tile * per), hi = min(a.n, lo + per);
    const uint32_t* sa = a.src_anc + (size_t)mv.src_k * a.n;
    uint32_t* da = a.dst_anc + (size_t)mv.dst_k * a.n;
    for (uint32_t i = lo + tid; i < hi; i += CSSM_FLEET_COPY_THREADS) da[i] = sa[i];
  }
  if (tile == 0u && tid < sizeof(FleetSeries) / 8u) {   // the scalars: ll, ess, err, fail_rec, next_ref
    const unsigned long long* ss = reinterpret_cast<const unsigned long long*>(a.src_ser + mv.src_k);
    unsigned long long* ds = reinterpret_cast<unsigned long long*>(a.dst_ser + mv.dst_k);
    ds[tid] = ss[tid];
  }
}
static_assert(sizeof(FleetSeries) % 8 == 0, "k_fleet_copy moves a FleetSeries as 8-byte words");

// one launch over `moves` table entries; 0 or the hipError_t
static int fleet_copy_launch(const FleetCopyArgs& a, uint32_t moves, hipStream_t stream) {
  if (!moves) return 0;
  hipLaunchKernelGGL(k_fleet_copy, dim3(moves * a.tiles), dim3(CSSM_FLEET_COPY_THREADS), 0, stream, a);
  return (int)hipGetLastError();
}
