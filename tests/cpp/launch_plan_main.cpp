// Stand-alone driver of the launch plan (csrc/cssm_launch_plan.cpp): a table of handle configurations -- the shapes at which a decision
// flips -- through the geometry, the propagate plan and the resampling plan behind it, for a build under -fsanitize=address,undefined
// (tests/test_launch_plan_host.py compiles and runs it, and compares what it prints with tests/golden/launch_plans.json).  No HIP, no
// device.  Every plan is held to what must be true of ANY plan (the EXPECTs below restate no threshold); one line per configuration of
// the table, "key => numbers", goes to stdout, and a denser sweep around the table is held to the invariants alone.  Exit status 0 =
// every expectation held.
#include <cstdio>
#include <cstring>

#include "cssm_launch_plan.h"

static int failures = 0;
static char key[256];
static bool pin = true;   // the configuration belongs to the pinned table: its plan is printed (else it is held to the invariants alone)
#define EXPECT(cond)                                                          \
  do {                                                                        \
    if (!(cond)) { std::printf("FAILED %s:%d: %s [%s]\n", __FILE__, __LINE__, #cond, key); ++failures; } \
  } while (0)

struct Cfg {
  uint64_t n = 0;
  int d = 1, rs = CSSM_RESAMPLE_SYSTEMATIC, fused = 1, whole = 0, wave = 1, grp = 1;
  uint32_t gmin = 0;   // 0: the handle's default
  int safe = 0, obs = CSSM_OBS_POISSON, lvl = 0, sharded = 0;
  uint64_t first = 0, n_global = 0;   // n_global 0: n
  int lsplit = 0;
  uint32_t umt = 4;
  int wp = 1, batch = 0, pick = 0, src2 = 0;
  size_t src2_stride = 0;
  int fsub = 0;
};

static void print_resample(const CssmResamplePlan& r) {
  std::printf(" %d %d %d %d %d %d", (int)r.tile_sums, r.lean_layout, r.tile_sums_flags, r.split, r.s2_par, (int)r.kernel);
}

static void run(const Cfg& q) {
  HostModel m;
  CssmLaunchFields c;
  m.d = q.d; m.obs_kind = q.obs; m.n_global = q.n_global ? q.n_global : q.n;
  c.n = q.n; c.first = q.first; c.sharded = q.sharded != 0;
  c.opt_fused = q.fused; c.opt_whole = q.whole; c.opt_wave = q.wave; c.opt_grp = q.grp;
  if (q.gmin) c.grp_min_units = q.gmin;
  c.resampler = q.rs; c.safe_sums = q.safe != 0; c.have_level = q.lvl != 0; c.wparity = q.wp; c.s2_par = 1;
  {   // the key: n, d and whatever differs from a default handle's first launch
    const Cfg def;
    int k = std::snprintf(key, sizeof key, "n=%llu d=%d", (unsigned long long)q.n, q.d);
    auto add = [&](const char* name, unsigned long long v, unsigned long long dv) { if (v != dv) k += std::snprintf(key + k, sizeof key - k, " %s=%llu", name, v); };
    add("resampler", q.rs, def.rs); add("fused", q.fused, def.fused); add("whole", q.whole, def.whole); add("wave", q.wave, def.wave); add("grp", q.grp, def.grp);
    add("grp_min_units", q.gmin, def.gmin); add("safe_sums", q.safe, def.safe); add("obs", q.obs, def.obs); add("have_level", q.lvl, def.lvl);
    add("sharded", q.sharded, def.sharded); add("first", q.first, def.first); add("n_global", q.n_global, def.n_global); add("lgcp_split", q.lsplit, def.lsplit);
    add("unit_max_tiles", q.umt, def.umt); add("wparity", q.wp, def.wp); add("batch", q.batch, def.batch); add("pick", q.pick, def.pick);
    if (q.src2) k += std::snprintf(key + k, sizeof key - k, " src2_stride=%zu", q.src2_stride);
    add("fsub", q.fsub, def.fsub);
  }

  cssm_plan_geometry(m, c, q.umt, q.lsplit);
  if (q.whole) c.split = 1;   // (cssm_pf_set_option: a CSSM_OPT_WHOLE_TILES other than 0 sets whole units)
  const uint64_t unit = (uint64_t)c.sup * CSSM_PLAN_TILE;
  EXPECT(c.stride == (size_t)c.ntiles * CSSM_PLAN_TILE && c.stride >= c.n && c.stride - c.n < CSSM_PLAN_TILE);
  EXPECT(c.sup >= 1 && (uint64_t)c.nunits * c.sup >= c.ntiles && (uint64_t)(c.nunits - 1) * c.sup < c.ntiles);
  EXPECT(c.split >= 1 && unit % c.split == 0);
  EXPECT(c.nsums >= c.ntiles && c.nsums >= (size_t)c.split * c.nunits);
  EXPECT(c.sharded ? c.nunits <= 1024u : true);

  CssmPropFacts f;
  f.batch = q.batch != 0; f.pick = q.pick != 0; f.src2 = q.src2 != 0; f.src2_stride = q.src2_stride; f.fsub = q.fsub != 0;
  const CssmPropPlan p = cssm_plan_propagate(m, c, f);
  EXPECT(p.grid >= 1 && (uint64_t)p.grid * p.chunk >= c.n && (uint64_t)(p.grid - 1) * p.chunk < c.n);
  EXPECT(p.chunk >= 1 && unit % p.chunk == 0);
  EXPECT(!p.want_ws || p.want_grp);
  EXPECT(!p.want_grp || p.do_sums);
  EXPECT(!p.want_ws || (4 * (size_t)c.nunits <= c.nsums && unit <= CSSM_PLAN_GRP_MAX_UNIT));
  EXPECT((p.grp_layout != 0) == p.want_grp && p.grp_layout >= 0 && p.grp_layout <= 2);
  EXPECT(p.grp_layout != 2 || (!c.sharded && !f.batch && c.nunits <= (uint32_t)(CSSM_PLAN_GRP_MAX * 64)));
  EXPECT((p.slot_set & ~CSSM_SLOT_SET_FIELDS) == 0);
  EXPECT(((p.slot_set & 0x100) != 0) == p.want_grp && ((p.slot_set & 0x2000) != 0) == p.want_ws);
  EXPECT(p.want_grp || (p.slot_set & ~0xff) == 0);
  EXPECT((p.slot_set & 0xff) < CSSM_PLAN_MAXSETS && ((p.slot_set >> 9) & 3) < CSSM_PLAN_MAXSETS);
  EXPECT(p.reduce == (p.geo == CSSM_GEO_FINE) && (!p.reduce || ((uint64_t)p.reduce_per_unit * p.chunk == unit && p.do_sums)));
  EXPECT(!p.reduce || (uint64_t)p.reduce_grid * (CSSM_PLAN_BLOCK / 64) >= c.nunits);
  EXPECT(p.one >= 0 && p.one <= 2 && (p.one != 1 || p.chunk == (uint64_t)CSSM_PLAN_BLOCK * cssm_prop_items(m.d)));
  EXPECT(!p.shard_slim || (c.sharded && p.do_sums));

  // the resampling launch behind that propagate, the dispatcher having honoured what the plan asked for; then the same observation redone
  c.last_optimistic = p.do_sums != 0; c.last_grp = p.want_grp; c.grp_layout = p.grp_layout; c.last_ws = p.want_ws;
  const CssmResamplePlan r = cssm_plan_resample(m, c, true, false);
  EXPECT(!cssm_offspring_is_wave(r.kernel) || p.want_ws);
  EXPECT(r.tile_sums == !p.do_sums && (r.tile_sums || r.lean_layout == 0) && (r.lean_layout != 0) == (r.tile_sums_flags != 0));
  EXPECT((r.tile_sums_flags & ~0x1f00) == 0 && r.split >= 1 && (r.s2_par == -1) == r.tile_sums);
  EXPECT(r.lean_layout != 2 || (!c.sharded && c.nunits <= (uint32_t)(CSSM_PLAN_GRP_MAX * 64)));
  const CssmResamplePlan w = cssm_plan_resample(m, c, true, true);   // (CSSM_NO_OFFW)
  EXPECT(!cssm_offspring_is_wave(w.kernel));
  c.safe_sums = true;
  const CssmPropPlan p2 = cssm_plan_propagate(m, c, CssmPropFacts());
  EXPECT(!p2.do_sums && !p2.want_grp && !p2.want_ws && !p2.reduce && (p2.slot_set & ~0xff) == 0);
  c.last_optimistic = false; c.last_grp = false; c.grp_layout = 0; c.last_ws = false;
  const CssmResamplePlan r2 = cssm_plan_resample(m, c, false, false);
  EXPECT(r2.tile_sums && r2.lean_layout == 0 && r2.tile_sums_flags == 0 && r2.s2_par == -1 && !cssm_offspring_is_wave(r2.kernel));

  if (!pin) return;
  std::printf("%s => %zu %u %u %u %u %zu | %d %d %llu %d %d %d %d %d %d %d %d %u %u |", key, c.stride, c.ntiles, c.sup, c.nunits, c.split, c.nsums, p.do_sums, p.geo,
              (unsigned long long)p.chunk, p.grid, p.one, p.slot_set, (int)p.want_grp, p.grp_layout, (int)p.want_ws, p.shard_slim, (int)p.reduce, p.reduce_grid,
              p.reduce_per_unit);
  print_resample(r);
  std::printf(" | %llu %d %d |", (unsigned long long)p2.chunk, p2.grid, p2.one);
  print_resample(r2);
  std::printf("\n");
}

int main() {
  const uint64_t ns[] = {1000, 100000, 1u << 18, (1u << 20) - 1024, 1u << 20, (1u << 20) + 1, 1u << 21, 1u << 22, (1u << 22) + 1024 /* > 1024 units: layout 2 */,
                         1u << 23, 1u << 24, (1u << 24) + 1024 /* > 4096 x 4 tiles: sup grows past 4 */};
  const int ds[] = {1, 2, 3, 4, 8, 9, 16};   // the edges of cssm_prop_items and CSSM_FINE_MIN_D
  for (uint64_t n : ns)
    for (int d : ds) {
      Cfg b; b.n = n; b.d = d;
      pin = true;    // the default handle: pinned at every size and dimension
      run(b);
      // one option or fact at a time: pinned at the sizes where the geometry changes and at the smallest and a large dimension, swept everywhere
      pin = (n == 100000 || n == 1u << 20 || n == 1u << 21 || n == (1u << 22) + 1024 || n == 1u << 24) && (d == 1 || d == 9);
      { Cfg q = b; q.rs = CSSM_RESAMPLE_STRATIFIED; run(q); }
      { Cfg q = b; q.rs = CSSM_RESAMPLE_MULTINOMIAL; run(q); }
      { Cfg q = b; q.fused = 0; run(q); }
      for (int w = 1; w <= 3; ++w) { Cfg q = b; q.whole = w; run(q); }
      { Cfg q = b; q.wave = 0; run(q); }
      { Cfg q = b; q.wave = 2; run(q); }
      { Cfg q = b; q.grp = 0; run(q); }
      { Cfg q = b; q.gmin = 1; run(q); }
      { Cfg q = b; q.gmin = 1; q.wave = 2; run(q); }
      { Cfg q = b; q.gmin = 1; q.batch = 1; run(q); }
      { Cfg q = b; q.safe = 1; run(q); }
      { Cfg q = b; q.obs = CSSM_OBS_LGCP; q.lvl = 0; run(q); }
      { Cfg q = b; q.obs = CSSM_OBS_LGCP; q.lvl = 1; run(q); }
      { Cfg q = b; q.obs = CSSM_OBS_LGCP; q.lvl = 1; q.fsub = 1; run(q); }
      { Cfg q = b; q.batch = 1; run(q); }
      { Cfg q = b; q.pick = 1; run(q); }
      { Cfg q = b; q.wp = 0; run(q); }
      { Cfg q = b; q.wp = 2; run(q); }
      { Cfg q = b; q.umt = 0; run(q); }
    }
  // shards: a quarter of the cloud each; an even and an odd first particle; the rows of an exchange read in place (stride 0) or from a buffer
  const uint64_t locals[] = {100000, 1u << 20, 1u << 21, 1u << 22, 1u << 24};
  const int sds[] = {1, 3, 9};
  for (uint64_t n : locals)
    for (int d : sds)
      for (uint64_t first : {(uint64_t)0, (uint64_t)1, n}) {
        Cfg b; b.n = n; b.d = d; b.sharded = 1; b.first = first; b.n_global = 4 * n;
        const bool mid = n >= 1u << 20 && n <= 1u << 22 && d != 3 && first <= 1;
        pin = mid;
        run(b);
        { Cfg q = b; q.src2 = 1; q.src2_stride = 0; run(q); }
        { Cfg q = b; q.src2 = 1; q.src2_stride = 4096; run(q); }
        { Cfg q = b; q.pick = 1; run(q); }
        pin = false;
        { Cfg q = b; q.grp = 0; run(q); }
        { Cfg q = b; q.gmin = 1; run(q); }
        { Cfg q = b; q.safe = 1; run(q); }
        { Cfg q = b; q.wp = 2; run(q); }
        for (int ls : {0, 1, 2, 4, 3}) {
          Cfg q = b; q.obs = CSSM_OBS_LGCP; q.lvl = 1; q.lsplit = ls;
          pin = mid && n >= 1u << 21 && d == 1 && first == 0;
          run(q);
          pin = pin && ls == 0;
          q.fsub = 1; run(q);
          q.fsub = 0; q.lvl = 0; run(q);
          q.lvl = 1; q.grp = 0; run(q);
        }
      }
  if (failures) { std::printf("launch_plan: %d expectation(s) failed\n", failures); return 1; }
  std::printf("launch_plan: ok\n");
  return 0;
}
