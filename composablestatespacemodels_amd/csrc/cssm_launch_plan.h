// cssm_launch_plan.h -- every launch decision of the single handle and of a shard as plain host code: the handle's geometry, the plan
// of one propagate launch and the plan of the resampling launch behind it.  Pure functions of a few integers, no device, no HIP header
// (cssm_launch_plan.cpp compiles with any host compiler, and under sanitizers with a main of its own: tests/cpp/launch_plan_main.cpp);
// cssm_pf.hip turns a plan and the handle's pointers into launches.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "cssm_records.h"

// The kernels' constants the decisions rest on, as cssm_device.hip.h and cssm_propagate.hip.h define them (a host-only file cannot
// include those): cssm_pf.hip, which sees both, asserts the equality.  The ones an experiment build overrides (-D in EXTRA) reach this file's
// translation unit too: the Makefile hands it EXTRA's definitions.
#define CSSM_PLAN_BLOCK 256
#define CSSM_PLAN_TILE 1024
#define CSSM_PLAN_MAXSETS 3
#define CSSM_PLAN_GRP_UNITS 32
#define CSSM_PLAN_GRP_MAX 64
#define CSSM_PLAN_GRP_SMALL 32
#define CSSM_PLAN_GRP_MAX_UNIT (1u << 15)
#ifdef CSSM_PROP_IT_LO
#define CSSM_PLAN_PROP_IT_LO CSSM_PROP_IT_LO
#else
#define CSSM_PLAN_PROP_IT_LO 2
#endif
#ifdef CSSM_PROP_IT_MID
#define CSSM_PLAN_PROP_IT_MID CSSM_PROP_IT_MID
#else
#define CSSM_PLAN_PROP_IT_MID 2
#endif
#ifndef CSSM_SPLIT_MAX_N
#define CSSM_SPLIT_MAX_N (1u << 20)
#endif
#ifndef CSSM_FINE_MIN_D
#define CSSM_FINE_MIN_D 4
#endif
#ifndef CSSM_LOOP_MAX_TILES
#define CSSM_LOOP_MAX_TILES 8
#endif

// What the decisions read of a handle beyond its model (HostModel: d, obs_kind, n_global).  cssm_pf (cssm_internal.h) derives from it,
// so a plan reads the handle itself and nothing is copied.
struct CssmLaunchFields {
  // sizes (cssm_plan_geometry fills stride .. nsums from the rest)
  uint64_t first = 0, n = 0;   // (n_global: HostModel)
  bool sharded = false;
  size_t stride = 0;
  uint32_t ntiles = 0;
  uint32_t sup = 1, nunits = 0;   // tiles per scan unit, number of units
  uint32_t split = 1;             // k_propagate blocks per unit (each owns a contiguous sub-unit and its sums)
  size_t nsums = 0;               // entries of the unit-sum arrays: a tile's or a sub-unit's each, whichever are more
  // options
  int opt_fused = 0;           // CSSM_OPT_FUSED_SUMS (set to 1 for sharded handles at creation)
  int opt_whole = 0;           // CSSM_OPT_WHOLE_TILES
  int opt_grp = 1;             // CSSM_OPT_GROUP_SUMS
  uint32_t grp_min_units = 2u * CSSM_PLAN_GRP_UNITS;   // smallest cloud (in units) whose propagate accumulates group sums (CSSM_GRP_MIN_UNITS: tests run small clouds through them)
  int opt_wave = 1;            // CSSM_OPT_WAVE_SUMS
  int resampler = CSSM_RESAMPLE_SYSTEMATIC;
  bool safe_sums = false;         // form the sums in their own pass after the max is known: the redo of an observation whose reference level the
                                  // max ruled out, cssm_pf_propagate (the host's resampler wants the log-weights), a shard's exported sums
  // what the launches so far left
  bool have_level = false;        // LGCP (contract v8): a weighted observation has run natively since the cloud was drawn / adopted -- its
                                  //   publisher left the next observation's predicted level (Scalars::next_ref), so the propagate may form the sums
  int wparity = 0;             // max-slot set (0 .. CSSM_MAXSETS - 1) of the next weighted step (single-GPU path); a shard: the set of GROUP
                               //   sums (Scalars::grp / grp2) of the next weighted observation -- its max slots stay in set 0
  int s2_par = 0;                 // buffer the next weighted observation's k_offspring writes
  bool last_optimistic = false;   // the last launch_propagate formed the sums itself (and stored weights in place of log-weights)
  bool last_grp = false;       // the last launch_propagate's blocks accumulated the sums of groups of units (Scalars::grp)
  int grp_layout = 0;          // ... in layout 1 (<= 32 groups of 32 units) or 2 (<= 64 groups of 64 units); 0: not at all
  bool last_ws = false;        // ... and its waves stored the exact sums of their quarter units (tileW): k_offspring_wave may run
};

int cssm_prop_items(int d);   // PropItems<D>

// stride, ntiles, sup, nunits, split and nsums of a handle of c.n particles.  unit_max_tiles: CSSM_UNIT_MAX_TILES (A/B; 4 unless set, 0: the
// old rule); shard_lgcp_split: CSSM_SHARD_LGCP_SPLIT (1, 2 or 4; anything else: the default of 2).
void cssm_plan_geometry(const HostModel& m, CssmLaunchFields& c, uint32_t unit_max_tiles, int shard_lgcp_split);
// ... its split alone, from the sizes (CSSM_OPT_WHOLE_TILES sets whole units and comes back to this)
uint32_t cssm_plan_split(const HostModel& m, const CssmLaunchFields& c, int shard_lgcp_split);

// whether the next propagate will use the kernels that also form the sums (and can record sampleOne's pick on the way) ...
bool cssm_uses_sums_kernel(const HostModel& m, const CssmLaunchFields& c);
// ... ever, in the series that is being enqueued (whether an observation can put it on hold)
bool cssm_may_use_sums_kernel(const CssmLaunchFields& c);
// the batched launches (cssm_batch.hip) serve this handle's configuration
int cssm_batch_ok(const HostModel& m, const CssmLaunchFields& c);

enum { CSSM_GEO_PIPE = 0, CSSM_GEO_LOOP = 1, CSSM_GEO_FINE = 2 };
int cssm_large_geometry(const HostModel& m, const CssmLaunchFields& c);

// The facts of one propagate call the plan needs besides the handle
struct CssmPropFacts {
  bool batch = false;        // a chain table is present (cssm_batch.hip)
  bool pick = false;         // the launch records sampleOne's pick
  bool src2 = false;         // candidates received from other ranks are read (a shard behind an exchange)
  size_t src2_stride = 0;    // ... at this stride (0: in place)
  bool fsub = false;         // a sub-step coefficient table is present (LGCP with a time-dependent f)
};
// slot_set, the set argument of the propagate kernels: bits 0-7 the max-slot set, bit 8 the blocks accumulate group sums, bits 9-10 the set
// of group sums, bits 11-12 log2(blocks per group / 32), bit 13 the waves store the sums of their quarter units
#define CSSM_SLOT_SET_FIELDS 0x3fff
struct CssmPropPlan {
  int do_sums;            // the kernels that also form the sums
  int geo;                // CSSM_GEO_*
  uint64_t chunk;         // particles per block
  int grid;
  int one;                // PropLaunch::one
  int slot_set;
  bool want_grp;          // bit 8 asked for; whether the kernel that runs honours it is the dispatcher's report
  int grp_layout;         // 1, 2, or 0 without want_grp
  bool want_ws;           // bit 13 asked for
  int shard_slim;         // PropLaunch::shard_slim
  bool reduce;            // k_reduce_units follows (CSSM_GEO_FINE): the blocks' sums -> the units'
  uint32_t reduce_grid, reduce_per_unit;   // ... on this grid, folding this many blocks per unit
};
CssmPropPlan cssm_plan_propagate(const HostModel& m, const CssmLaunchFields& c, const CssmPropFacts& f);

// The instantiation the resampling launch runs: k_offspring_wave<GRPL> or k_offspring_self<RS, RAWC, GRP>
enum CssmOffspringKernel {
  CSSM_OFF_WAVE_1, CSSM_OFF_WAVE_2,                                      // behind a propagate that stored its waves' sums (layout 1 / 2)
  CSSM_OFF_SELF_SYS_FUSED_GRP1, CSSM_OFF_SELF_SYS_FUSED_GRP2,            // <SYSTEMATIC, 2, 1 / 2>: behind a fused-sums propagate with group sums
  CSSM_OFF_SELF_SYS_FUSED, CSSM_OFF_SELF_STRAT_FUSED, CSSM_OFF_SELF_MULTI_FUSED,   // <RS, 2>
  CSSM_OFF_SELF_SYS_GRP1, CSSM_OFF_SELF_SYS_GRP2,                        // <SYSTEMATIC, 0, 1 / 2>: behind k_tile_sums with group sums
  CSSM_OFF_SELF_SYS, CSSM_OFF_SELF_STRAT, CSSM_OFF_SELF_MULTI            // <RS, 0>
};
static inline bool cssm_offspring_is_wave(CssmOffspringKernel k) { return k == CSSM_OFF_WAVE_1 || k == CSSM_OFF_WAVE_2; }
struct CssmResamplePlan {
  bool tile_sums;         // k_tile_sums runs first (the propagate stored log-weights)
  int lean_layout;        // ... adding the units' sums to their groups' in this layout (0: not)
  int tile_sums_flags;    // ... told so by this word (bits 8-12 of slot_set)
  int split;              // sub-units per unit k_offspring scans
  int s2_par;             // the buffer of partial sums of squares it writes (-1: none, the ESS is formed at once)
  CssmOffspringKernel kernel;
};
// allow_grp = false: a REDONE observation -- the set of group sums it would add to still holds the sums of its first attempt.
// no_offw: CSSM_NO_OFFW (A/B: k_offspring_self behind the wave-range propagate)
CssmResamplePlan cssm_plan_resample(const HostModel& m, const CssmLaunchFields& c, bool allow_grp, bool no_offw);
