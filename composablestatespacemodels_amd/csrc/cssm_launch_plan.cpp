// cssm_launch_plan.cpp -- the launch decisions of cssm_launch_plan.h.  Host only: no HIP header, no device, no global state.
#include "cssm_launch_plan.h"

// k_offspring_wave keeps the deferred chunks of a wave's quarter unit in a 32-bit map (cssm_offspring_wave.hip.h, beside `cold`, asserts
// the same): a quarter tile per chunk, at most 32 of them while a unit has at most CSSM_GRP_MAX_UNIT particles -- the bound want_grp,
// and through it want_ws, holds below
static_assert(CSSM_PLAN_TILE / 4 == 256 && CSSM_PLAN_GRP_MAX_UNIT / CSSM_PLAN_TILE <= 32, "a wave's quarter unit has at most 32 chunks of 256 particles");

int cssm_prop_items(int d) { return d <= 2 ? CSSM_PLAN_PROP_IT_LO : (d <= 8 ? CSSM_PLAN_PROP_IT_MID : 1); }   // PropItems<D>

// ------------------------------------------------------------------------------------ the handle's geometry

// k_propagate blocks per 1024-particle unit on a single-GPU handle: one tile of the kernel per block below 2^20 particles
uint32_t cssm_plan_split(const HostModel& m, const CssmLaunchFields& c, int shard_lgcp_split) {
  // (measured and dropped: a shard of an LGCP filter on blocks of 1024 particles where a unit has 2048 -- k_propagate 71.8 -> 68.4 us at
  //  2^21 particles per rank, one round of whole-unit blocks running in lockstep being 12 % slower per particle than the same kernel on
  //  several rounds; but the exchange kernel's header and prefix blocks, which every block of every rank waits for, then total twice
  //  the sums: 18.5 -> 20.4 us, the step 89.5 -> 90.3)
  if (c.sharded) {
    // an LGCP shard whose units have several tiles: blocks of HALF a unit -- whole-unit blocks all start together (1024 of them, one
    // round) and run in lockstep, so every memory wait of the prologue and of the tile boundaries is exposed; half-unit blocks run in
    // two staggered rounds (k_propagate 71.8 -> 68.4 us at 2^21 particles per rank).  The exchange kernels do not see the difference
    // any more: they read the sums of groups of units (Scalars::grp), to which every block adds its own.  CSSM_SHARD_LGCP_SPLIT: 1, 2, 4.
    if (m.obs_kind != CSSM_OBS_LGCP || c.sup < 2) return 1u;
    uint32_t want = 2u;
    { const int v = shard_lgcp_split; if (v == 1 || v == 2 || v == 4) want = (uint32_t)v; }
    // (whole tiles of 1024: the exchange's pack blocks take the prefix of a boundary block's tiles from the blocks' sums only then --
    //  quarter-unit blocks of 512 particles at 2^21 per rank sent them down their recompute path: 39 us per exchange)
    while (want > 1u && ((uint64_t)c.sup * CSSM_PLAN_TILE / want) % (uint64_t)CSSM_PLAN_TILE != 0) want >>= 1;
    const uint64_t unit_particles = (uint64_t)c.sup * CSSM_PLAN_TILE;
    if (!(c.opt_grp && c.nunits >= c.grp_min_units && c.nunits <= (uint32_t)(CSSM_PLAN_GRP_SMALL * CSSM_PLAN_GRP_UNITS) && unit_particles <= CSSM_PLAN_GRP_MAX_UNIT)) want = 1u;   // (no group sums: whole units)
    return want;
  }
  if (c.sup != 1 || c.n >= CSSM_SPLIT_MAX_N) return 1u;
  return cssm_prop_items(m.d) == 1 ? 4u : 2u;   // one tile of the kernel: half of 1024 (two particles per thread), a quarter (one)
}

void cssm_plan_geometry(const HostModel& m, CssmLaunchFields& c, uint32_t unit_max_tiles, int shard_lgcp_split) {
  c.stride = (size_t)((c.n + CSSM_PLAN_TILE - 1) / CSSM_PLAN_TILE) * CSSM_PLAN_TILE;   // rows start 16-B aligned
  c.ntiles = (uint32_t)((c.n + CSSM_PLAN_TILE - 1) / CSSM_PLAN_TILE);
  c.sup = (c.ntiles + 1023u) / 1024u;
  // Single GPU, clouds beyond 2^22 particles: units of 4 tiles while that gives at most 4096 of them (2^23: 2048 units, 2^24: 4096), larger
  // units beyond -- instead of 1024 units of ever more tiles (16 at 2^24: 1025 k_offspring blocks walking 16 tiles each through three
  // barriers per tile, 1024 k_propagate blocks on 1536 resident slots at d = 1).  k_offspring finds its prefix through the sums of up
  // to 64 groups of 64 units (Scalars::grp, layout 2).  A shard keeps at most 1024 units (its exchange kernels' geometry).
  // CSSM_UNIT_MAX_TILES (A/B): the tiles per unit to aim for (default 4; 0: the old rule).
  if (!c.sharded && c.sup > 4u) {
    const uint32_t want = unit_max_tiles;
    if (want >= 1u) {
      const uint32_t least = (c.ntiles + (uint32_t)(CSSM_PLAN_GRP_MAX * 64) - 1u) / (uint32_t)(CSSM_PLAN_GRP_MAX * 64);   // at most 4096 units
      const uint32_t sup2 = want > least ? want : least;
      if (sup2 < c.sup) c.sup = sup2;
    }
  }
  c.nunits = (c.ntiles + c.sup - 1) / c.sup;
  // k_propagate: a block owns unit/split particles, a multiple of its CSSM_BLOCK * IT particles per iteration
  // (the kernel pipelines its tiles through LDS and wants several of them: one block per unit)
  // Clouds below 2^20 particles on one GPU: one tile of the kernel per block.  Up to ~2^18 particles every SIMD holds at
  // most one or two waves and a kernel's duration is the length of ONE wave's dependent instruction stream (~3 ns per
  // instruction, tools/launch_floor.hip; the launch itself is 3.1 us): one pair of particles per thread instead of two, in the
  // single-tile instantiation k_propagate_self<..., ONE> that requests everything position-dependent in its first round of
  // loads and draws its normals while the gathered rows travel.  Per observation, bench model, same process (tools/ab_fine.py):
  // 17.1 -> 12.6 us at N = 100 000, 21.9 -> 19.3 at 2^19, 28.1 -> 25.8 at 3 * 2^18.  From 2^20 particles on: whole units per
  // block (cssm_plan_propagate).
  c.split = cssm_plan_split(m, c, shard_lgcp_split);
  c.nsums = (size_t)(c.ntiles > 4 * c.nunits ? c.ntiles : 4 * c.nunits);   // (up to four sub-units per unit)
}

// ------------------------------------------------------------------------------------ the propagate launch

// (LGCP, contract v8: once a weighted observation has run natively its max predicts the next one's level -- Scalars::next_ref --
//  and the sums are formed inside the propagate like everybody else's; the first observation's level is its max)
bool cssm_uses_sums_kernel(const HostModel& m, const CssmLaunchFields& c) {
  return c.opt_fused && !c.safe_sums && (m.obs_kind != CSSM_OBS_LGCP || c.have_level) && c.resampler != CSSM_RESAMPLE_MULTINOMIAL;
}
bool cssm_may_use_sums_kernel(const CssmLaunchFields& c) {
  return c.opt_fused && !c.safe_sums && c.resampler != CSSM_RESAMPLE_MULTINOMIAL;
}

// Launch geometry of the sums kernels on clouds of 2^20 particles and more (one GPU; whole units of 1024 * sup particles).
// In-process A/B (tools/ab_opt.py option 6, tools/ab_fine.py; per observation; boxes of this pool differ by +-5 %, only runs of
// one process compare):
//   LOOP    one block per unit running the single-tile-style kernel tile after tile (k_propagate_self<..., ONE>: no software-
//           pipeline state, no spill, 5-6 waves per SIMD; co-resident waves cover the round trips).  While a block has at most
//           CSSM_LOOP_MAX_TILES tiles it beats everything else: d = 3: 31.0 vs 33.2 (half tiles) / 32.5 (pipelined) us at 2^20,
//           50.7 vs 53.3 at 2^21, 90.0 vs 93.0 at 2^22, a tie at 2^23, 376 vs 368 at 2^24; d = 1: 23.6 vs 26.9 at 2^20, a tie at 2^22,
//           252 vs 241 at 2^24; d = 4: 108 vs 120 at 2^22; d = 9: 57.6 vs 63.4 at 2^20, 105 vs 114 at 2^21; d = 16 at 2^22 (16 tiles): 329 vs 313.
//   FINE    one tile per block + k_reduce_units (~5 us): larger clouds of d >= 4 (d = 9: 194 vs 203 us pipelined at 2^22; d = 16: 287 vs 343)
//   PIPE    one block per unit, the software-pipelined kernel: larger clouds of d <= 3 (a tie with FINE at d = 3, a few per cent better at d <= 2)
int cssm_large_geometry(const HostModel& m, const CssmLaunchFields& c) {
  if (c.sharded || c.split != 1 || c.first != 0 || c.n != m.n_global || c.resampler == CSSM_RESAMPLE_MULTINOMIAL) return CSSM_GEO_PIPE;
  if (c.opt_whole == 1) return CSSM_GEO_LOOP;
  if (c.opt_whole == 2) return CSSM_GEO_PIPE;
  if (c.opt_whole == 3) return CSSM_GEO_FINE;
  const uint32_t tiles = c.sup * (uint32_t)CSSM_PLAN_TILE / (uint32_t)(CSSM_PLAN_BLOCK * cssm_prop_items(m.d));
  if (tiles <= CSSM_LOOP_MAX_TILES) return CSSM_GEO_LOOP;
  return m.d >= CSSM_FINE_MIN_D ? CSSM_GEO_FINE : CSSM_GEO_PIPE;
}

int cssm_batch_ok(const HostModel& m, const CssmLaunchFields& c) {
  return c.opt_fused && !c.safe_sums && m.obs_kind != CSSM_OBS_LGCP && c.resampler == CSSM_RESAMPLE_SYSTEMATIC && !c.sharded &&
         cssm_large_geometry(m, c) != CSSM_GEO_FINE;
}

CssmPropPlan cssm_plan_propagate(const HostModel& m, const CssmLaunchFields& c, const CssmPropFacts& f) {
  CssmPropPlan p;
  // one block per sub-unit: contiguous ranges, so that (with do_sums) the block's fixed-point sums are the
  // sub-unit sums k_offspring scans
  uint64_t chunk = (uint64_t)c.sup * CSSM_PLAN_TILE / c.split;
  const int do_sums = cssm_uses_sums_kernel(m, c) ? 1 : 0;
  const int geo = do_sums ? cssm_large_geometry(m, c) : CSSM_GEO_PIPE;
  const bool fine = geo == CSSM_GEO_FINE;
  const uint64_t unit_particles = (uint64_t)c.sup * CSSM_PLAN_TILE;
  if (fine) chunk = (uint64_t)CSSM_PLAN_BLOCK * cssm_prop_items(m.d);   // (divides the unit: 1024 * sup)
  const int grid = (int)((c.n + chunk - 1) / chunk);
  const bool lgcp = m.obs_kind == CSSM_OBS_LGCP;
  p.do_sums = do_sums; p.geo = geo; p.chunk = chunk; p.grid = grid;
  p.slot_set = c.sharded ? 0 : c.wparity;
  // one fused-sums block per unit of a single-GPU cloud: the blocks also accumulate the sums of groups of 32 units (Scalars::grp,
  // bit 8 of the set argument of k_propagate_self and k_offspring_self), which k_offspring then reads instead of every unit sum
  // (a shard: the same, in Scalars::grp and grp2 -- both sums travel in the exchange's headers --, the set rotating with the handle's
  //  weighted observations while its max slots stay in set 0; the exchange kernels read 32 group sums instead of every unit sum)
  // layout 1: at most 32 groups of 32 units; layout 2 (single GPU, not the batched chains): at most 64 groups of 64 units
  const bool big = c.nunits > (uint32_t)(CSSM_PLAN_GRP_SMALL * CSSM_PLAN_GRP_UNITS);
  const bool want_grp = do_sums && !fine && chunk * c.split == unit_particles && (c.sharded ? c.split <= 4u : (c.split == 1 && c.first == 0 && c.n == m.n_global)) &&
                        c.nunits >= c.grp_min_units && (big ? (!c.sharded && !f.batch && c.nunits <= (uint32_t)(CSSM_PLAN_GRP_MAX * 64)) : true) &&
                        unit_particles <= CSSM_PLAN_GRP_MAX_UNIT && c.opt_grp;
  p.want_grp = want_grp;
  p.grp_layout = want_grp ? (big ? 2 : 1) : 0;
  // bits 11-12: log2(blocks per group / 32) -- the blocks per unit of a shard's split launch, or the 64-unit groups of layout 2
  if (want_grp) p.slot_set |= 0x100 | (c.wparity << 9) | ((big ? 1 : (c.split == 4u ? 2 : (c.split == 2u ? 1 : 0))) << 11);
  // ... and, on the single GPU's tile-after-tile launch behind systematic resampling, the exact sums of the waves' quarter units (bit 13;
  // the array travels in the slot of the sums of squares, which these kernels leave to k_offspring): k_offspring_wave then needs neither
  // a conversion nor a 128-bit scan per weight (CSSM_OPT_WAVE_SUMS = 0: k_offspring_self as before).  want_grp's bound on the unit
  // (unit_particles <= CSSM_GRP_MAX_UNIT) is also what k_offspring_wave's map of deferred chunks rests on: the static_assert above.
  const bool want_ws = want_grp && geo == CSSM_GEO_LOOP && !c.sharded && !f.batch && c.resampler == CSSM_RESAMPLE_SYSTEMATIC &&
                       m.obs_kind != CSSM_OBS_LGCP && !f.pick && 4 * (size_t)c.nunits <= c.nsums &&
                       // (where it pays: units of several tiles -- clouds beyond 2^20 particles: at one tile per unit the resampling kernel gains
                       //  nothing back -- and at most two latent components: a block on wave ranges streams 4 x (d rows + weights) ranges instead
                       //  of d + 1, and from d = 3 on the propagate loses to that what the resampling kernel gains (same-box A/B of round 6: the
                       //  step -1.2 % on slower boxes, +0-5 % on the fastest, where the block-wide propagate runs at 0.68 of the HBM peak; d = 1:
                       //  -4.8 % .. 0).  CSSM_OPT_WAVE_SUMS = 2 forces it wherever the geometry allows.)
                       (c.opt_wave == 2 || (c.opt_wave != 0 && c.sup >= 2u && m.d <= 2));
  p.want_ws = want_ws;
  if (want_ws) p.slot_set |= 0x2000;
  p.one = (chunk == (uint64_t)CSSM_PLAN_BLOCK * cssm_prop_items(m.d)) ? 1 : (geo == CSSM_GEO_LOOP ? 2 : 0);
  // sharded handle on the single-collective exchange (received rows read in place: src2_stride == 0) or before its first exchange:
  // slim launch, tile after tile while a unit has at most CSSM_LOOP_MAX_TILES tiles; whole pairs per thread (d <= 8) need an even first id
  p.shard_slim = c.sharded && do_sums && !lgcp && (!f.src2 || f.src2_stride == 0) && !f.fsub && !f.pick &&
                 ((c.first & 1ull) == 0ull || cssm_prop_items(m.d) == 1) && (p.slot_set & 0xff) == 0;
  if (p.shard_slim && c.sup * (uint32_t)CSSM_PLAN_TILE / (uint32_t)(CSSM_PLAN_BLOCK * cssm_prop_items(m.d)) <= CSSM_LOOP_MAX_TILES) p.one = 2;
  // the blocks' sums -> the units' (the kernel itself skips unweighted observations and series on hold)
  p.reduce = fine;
  p.reduce_grid = (c.nunits + CSSM_PLAN_BLOCK / 64 - 1) / (CSSM_PLAN_BLOCK / 64);
  p.reduce_per_unit = (uint32_t)(unit_particles / chunk);
  return p;
}

// ------------------------------------------------------------------------------------ the resampling launch

CssmResamplePlan cssm_plan_resample(const HostModel& m, const CssmLaunchFields& c, bool allow_grp, bool no_offw) {
  CssmResamplePlan p;
  const bool optimistic = c.last_optimistic;
  p.split = optimistic ? (int)c.split : 1;
  // the sums as a pass of their own on a cloud of many units (systematic resampling, one GPU): k_tile_sums adds the units' sums to their
  // groups' too, and k_offspring_self<..., 0, GRP> finds its prefix through those instead of every block reading every unit sum (at
  // 4096 units: 64 KiB per block, 100 us per launch at N = 2^24 against 67)
  int lean_layout = 0;
  if (!optimistic && allow_grp && !c.sharded && c.opt_grp && c.resampler == CSSM_RESAMPLE_SYSTEMATIC && c.first == 0 && c.n == m.n_global &&
      c.nunits >= c.grp_min_units && c.nunits <= (uint32_t)(CSSM_PLAN_GRP_MAX * 64) && (uint64_t)c.sup * CSSM_PLAN_TILE <= CSSM_PLAN_GRP_MAX_UNIT)
    lean_layout = c.nunits > (uint32_t)(CSSM_PLAN_GRP_SMALL * CSSM_PLAN_GRP_UNITS) ? 2 : 1;
  p.tile_sums = !optimistic;
  p.lean_layout = lean_layout;
  p.tile_sums_flags = lean_layout ? (0x100 | (c.wparity << 9) | ((lean_layout == 2 ? 1 : 0) << 11)) : 0;
  p.s2_par = optimistic ? c.s2_par : -1;
  const int rs = c.resampler;
  const bool sys = rs == CSSM_RESAMPLE_SYSTEMATIC;
  if (optimistic && c.last_grp && c.last_ws && !no_offw && sys) p.kernel = c.grp_layout == 2 ? CSSM_OFF_WAVE_2 : CSSM_OFF_WAVE_1;
  else if (optimistic && c.last_grp && c.grp_layout == 2 && sys) p.kernel = CSSM_OFF_SELF_SYS_FUSED_GRP2;
  else if (optimistic && c.last_grp && sys) p.kernel = CSSM_OFF_SELF_SYS_FUSED_GRP1;
  else if (optimistic) p.kernel = sys ? CSSM_OFF_SELF_SYS_FUSED : (rs == CSSM_RESAMPLE_STRATIFIED ? CSSM_OFF_SELF_STRAT_FUSED : CSSM_OFF_SELF_MULTI_FUSED);
  else if (lean_layout == 2 && sys) p.kernel = CSSM_OFF_SELF_SYS_GRP2;
  else if (lean_layout == 1 && sys) p.kernel = CSSM_OFF_SELF_SYS_GRP1;
  else p.kernel = sys ? CSSM_OFF_SELF_SYS : (rs == CSSM_RESAMPLE_STRATIFIED ? CSSM_OFF_SELF_STRAT : CSSM_OFF_SELF_MULTI);
  return p;
}
