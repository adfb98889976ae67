// cssm_internal.h -- what the HIP translation units of libcssm_pf share: the handle, error plumbing and the launch helpers
// that both the single-GPU drivers (cssm_pf.hip) and the sharded stages (cssm_shard.hip) use.  Not part of the C ABI.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstring>
#include <string>
#include <vector>

#include "cssm_host.h"
#include "cssm_launch_plan.h"
#include "cssm_window.h"

#define fail cssm_fail
#define HIP_TRY(expr)                                                                         \
  do {                                                                                        \
    hipError_t e__ = (expr);                                                                  \
    if (e__ != hipSuccess) return fail(CSSM_EHIP, "%s: %s (%s:%d)", #expr, hipGetErrorString(e__), __FILE__, __LINE__); \
  } while (0)


// What one call borrows from the device -- memory, events, a stream: made through this owner, released when it goes out of scope,
// on every path out of the function.  (The handles' long-lived buffers are not its business.)
struct CssmTemps {
  std::vector<void*> mem;
  std::vector<hipEvent_t> events;
  hipStream_t own_stream = nullptr;
  CssmTemps() = default;
  CssmTemps(const CssmTemps&) = delete;
  CssmTemps& operator=(const CssmTemps&) = delete;
  ~CssmTemps() {
    for (hipEvent_t e : events) (void)hipEventDestroy(e);
    for (void* p : mem) (void)hipFree(p);
    if (own_stream) (void)hipStreamDestroy(own_stream);
  }
  template <class T>
  hipError_t alloc(T*& p, size_t bytes) {
    void* q = nullptr;
    const hipError_t e = hipMalloc(&q, bytes);
    if (e == hipSuccess) { mem.push_back(q); p = static_cast<T*>(q); }
    return e;
  }
  hipError_t event(hipEvent_t& ev) {
    const hipError_t e = hipEventCreate(&ev);
    if (e == hipSuccess) events.push_back(ev);
    return e;
  }
  hipError_t stream(hipStream_t& st) {
    const hipError_t e = hipStreamCreateWithFlags(&st, hipStreamNonBlocking);
    if (e == hipSuccess) own_stream = st;
    return e;
  }
};
// a failed allocation through the owner `tmp`: CSSM_ENOMEM (every other HIP error: HIP_TRY)
#define HIP_ALLOC(tmp, p, bytes)                                                                                   \
  do {                                                                                                             \
    if ((tmp).alloc(p, (bytes)) != hipSuccess) return fail(CSSM_ENOMEM, "hipMalloc(%zu) for " #p " (%s:%d)", (size_t)(bytes), __FILE__, __LINE__); \
  } while (0)

#define CSSM_NKERNELS CSSM_PROFILE_NKERNELS


// (CssmLaunchFields: the sizes, options and running state every launch decision reads -- cssm_launch_plan.h)
struct cssm_pf : HostModel, CssmLaunchFields {
  int device = 0;
  int n_cus = 256;             // compute units of the device (launch geometry decisions)
  hipStream_t stream = nullptr;
  bool own_stream = true;
  bool wmode = false;             // the log-weight buffer holds the WEIGHTS exp(min(w - c, 2^-20)) of the last weighted observation
  bool sums_ready = false;        // sharded: the unit sums of the last propagated observation exist (k_propagate<SUMS> or cssm_pf_shard_sums)
  // ESS pending (Scalars::pend): k_offspring's blocks leave partial sums of squared weights in s2buf[par * s2_stride + block]
  cssm_u128* s2buf = nullptr;     // 2 x s2_stride entries
  uint32_t s2_stride = 0;          // (= nsums)
  uint32_t gen = 0;               // generation of the batch call / streaming step that owns d_ess_t
  int32_t ess_host = 0;           // ESS of the last completed observation as the host knows it
  void* last_comm = nullptr;      // RCCL communicator the library last enqueued collectives on (bounded_sync)
  std::vector<double> h_fsub;     // host copy of the sub-step coefficient table of the records last built
  double* d_fsub = nullptr; size_t fsub_cap = 0;
  // device memory
  double* state[2] = {nullptr, nullptr};
  int cur = 0;                 // state[cur] = propagated cloud of the last step (x1)
  const double* src = nullptr; // where the next propagate reads (state[cur])
  size_t src_stride = 0;
  const double* src2 = nullptr; // sharded: candidates received from other ranks (indices >= n_split)
  size_t src2_stride = 0;
  uint32_t n_split = 0;
  double* logw = nullptr;
  uint32_t* endslot = nullptr;
  uint32_t* anc = nullptr;
  bool anc_valid = false;
  int opt_exact = 0;           // CSSM_OPT_EXACT_OFFSPRING
  cssm_u128 *fineS = nullptr, *fineS2 = nullptr;   // large clouds: the sums of k_propagate's single-tile blocks (k_reduce_units folds them into tileS / tileS2)
  size_t fine_cap = 0;
  int opt_spec = 1;            // CSSM_OPT_SPECIALISE
  cssm_u128* tileW = nullptr;  // four per unit: the quarter units' sums (k_propagate_self<..., SUMS = 1, ONE = 2>, bit 13 of its set argument)
  double* cum = nullptr;       // multinomial: cumulative normalised weights
  const long long *send_first_dev = nullptr, *send_count_dev = nullptr;   // last shard_offspring outputs (device)
  cssm_u128 *tileS = nullptr, *tileS2 = nullptr, *tileP = nullptr;
  cssm_u128* unitPre = nullptr;   // sharded, single-collective exchange: exclusive prefixes of the unit sums (k_boundary_pack -> k_offspring_expand_spec)
  bool spec_pre = false;          // ... written by the last cssm_pf_shard_boundary_pack
  Scalars* sc = nullptr;
  double *d_m0 = nullptr, *d_sd0 = nullptr, *d_logtab = nullptr;
  StepRec* d_recs = nullptr;
  size_t recs_cap = 0;
  double* d_ll_t = nullptr;
  int32_t* d_ess_t = nullptr;
  // host-mapped mirrors k_finish writes at the end of a call (the host synchronises the stream and reads them: no D2H copy)
  double* h_ll_t = nullptr; double* hd_ll_t = nullptr;       // host pointer / the same memory as the device sees it
  int32_t* h_ess_t = nullptr; int32_t* hd_ess_t = nullptr;
  Scalars* hd_sc = nullptr;                                   // device view of h_sc
  double* d_path = nullptr;
  size_t path_cap = 0;
  // sharded extras
  double* cand = nullptr;      // candidate states received for this rank, SoA [d][cand_cap]
  size_t cand_cap = 0;
  uint32_t *cand_end = nullptr, *cand_idx = nullptr;   // end slot / state index of every candidate, global order
  size_t cidx_cap = 0;
  int64_t* d_bounds = nullptr;
  int64_t* d_xch = nullptr;    // exact exchange: [0..63] send first, [64..127] send count; [128] the redo flag k_offspring_expand_spec writes
  uint32_t* d_need = nullptr;  // per observation: rows the exchange needed (diagnostics of cssm_pf_shard_status; zero since the
  size_t need_cap = 0;         //   two-collective exchange that recorded them was removed)
  bool series = false;         // records of a whole series are resident (cssm_pf_shard_begin / _continue)
  // sharded cloud summaries (cssm_pf_shard_summary_*): keys of the local cloud, block partial sums, the two radix-select states per row
  unsigned long long* sm_keys = nullptr; double* sm_partial = nullptr; void* sm_st = nullptr; StepRec* sm_rec = nullptr;
  size_t sm_cap = 0; int sm_blocks = 0; double sm_time = 0.0;
  // peer-written exchange (cssm_shard.hip: PeerState; the device table and the ticket counters k_boundary_pack uses)
  void* peer = nullptr; void* peer_tab = nullptr; unsigned int* peer_tickets = nullptr;
  unsigned long long peer_wait_ticks = 3000000000ull;   // 30 s of the 100 MHz clock (CSSM_PEER_TIMEOUT_MS): Scalars::peer_wait_ticks
  uint32_t peer_seq = 0;       // number of the last exchange enqueued on the peer windows (window = seq & 1; the flags carry it)
  uint32_t peer_probe_plain_bad = 0;   // cssm_pf_shard_peer_probe_stale
  bool peer_packed = false;    // cssm_pf_shard_pack_peer ran, cssm_pf_shard_adopt_peer has not yet
  bool peer_rows_packed = false;   // ... and cssm_pf_shard_pack_rows_peer (the second stage of a pack that sends the needed rows only)
  bool peer_all_rows = false;  // CSSM_PEER_ALL_ROWS=1: every row of the boundary blocks travels (else the eager rows + what the neighbour's slots need beyond them)
  long long peer_eager = 4096; // CSSM_PEER_EAGER_ROWS: rows next to the boundary that travel at once, ahead of the headers (four tiles)
  bool want_path = false;      // sharded `filter`: record sampleOne's pick after every observation whose slot this rank owns
  uint32_t rec_base = 0;       // observation index (pf->step) of the resident series' first record: 0 after _begin, the filter's
                               //   observation count so far after _continue
  struct Snap { int cur; const double* src; size_t src_stride; const double* src2; size_t src2_stride; uint32_t n_split; bool anc_valid, last_optimistic; uint32_t step; double t; bool have_level;
                int wparity; bool last_grp; };   // (the set of group sums the observation's propagate added to, and whether it did)
  std::vector<Snap> snaps;     // host-side state right after the propagate of every observation of the series (cssm_pf_shard_resume)
  std::vector<Snap> pre_snaps; // ... and right BEFORE it (cssm_pf_shard_resume_level: the observation is propagated again)
  // host staging (pinned)
  StepRec* h_recs = nullptr;
  StepRec* h_recs_dev = nullptr;   // the device's address of h_recs (k_fetch_recs)
  size_t h_recs_cap = 0;
  Scalars* h_sc = nullptr;     // pinned: the streaming step's scalars land here without a staging copy
  // filter state
  double t = 0.0;
  uint32_t step = 0;
  uint32_t h_step_for_resample = 0;   // observation index of the step being resampled (Philox counter word)
  bool initialised = false;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  float last_ms = -1.f;
  int opt_events = 0;              // CSSM_OPT_LOOP_EVENTS: the batch drivers bracket their device loop with an event pair
  bool have_events = false;        // ... and the last call did
  // optional per-kernel timing (HIP events on the launch stream around every kernel)
  bool profile = false;
  uint32_t* h_done = nullptr; uint32_t* hd_done = nullptr; uint32_t done_seq = 0;   // k_finish's completion word (host-mapped), read_scalars polls it
  std::vector<hipEvent_t> prof_ev;         // pairs
  std::vector<int> prof_kind;              // kernel kind of pair i
  size_t prof_used = 0;
  double prof_ms[CSSM_NKERNELS] = {0};
  uint64_t prof_cnt[CSSM_NKERNELS] = {0};
  // forecasts (cssm_forecast.hip): the leftmost leaf's scale as stored (BetaModel.observation takes it as it is), the key-buffer cap
  // (CSSM_OPT_FORECAST_CAP; 0 = 1 GiB) and the device times of the last call (cssm_pf_forecast_last_ms; < 0: none yet)
  int obs_has_scale = 0;
  double obs_scale = 0.0;
  size_t forecast_cap = 0;
  double forecast_ms[2] = {-1.0, -1.0};
  // cssm_pf_smooth (cssm_smooth.hip): the slots per block tile of its backward kernels (CSSM_OPT_SMOOTH_TILE; 0 = CSSM_SMOOTH_TILE) and
  // the device times of the last call (cssm_pf_smooth_last_ms; < 0: none yet)
  uint32_t smooth_tile = 0;
  double smooth_ms[3] = {-1.0, -1.0, -1.0};
  // cssm_pf_filter_intervals (cssm_intervals.hip): the selection's scratch, the call's row buffer and its timing (IvScratch; made at the
  // first call, freed by cssm_iv_free)
  void* iv = nullptr;
  // cssm_pf_filter_forecasts (cssm_intervals.hip): the same for its rows of d + 2 (a sibling IvScratch)
  void* fc = nullptr;
  // cssm_pf_window / cssm_pf_step_interpolate (cssm_intervals.hip): the ring's bookkeeping (cssm_window.h; slices = 0: no window), the ring
  // itself with its slices' times (PfWindow) and the selection's scratch of the lineage rows (a third IvScratch).  Every call that writes
  // the cloud, the key or the parameters restarts the window: three integer stores, whether a window is open or not.
  cssm_window wring = {0u, 0u, 0u};
  void* win = nullptr;
  void* li = nullptr;
  // cssm_pf_if2 (cssm_if2.hip): where the flattened vector of the descriptor the handle was created with holds what a component reads
  // (not built for an LGCP handle, which the call refuses), and the device time of the last call (cssm_pf_if2_last_ms; < 0: none yet)
  If2Map if2_map;
  bool if2_map_ok = false;
  double if2_ms = -1.0;
};

// begin/end of one profiled launch
static inline void prof_begin(cssm_pf* pf, int kind) {
  if (!pf->profile) return;
  if (pf->prof_used * 2 + 2 > pf->prof_ev.size()) {
    hipEvent_t a, b;
    if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) { pf->profile = false; return; }
    pf->prof_ev.push_back(a); pf->prof_ev.push_back(b);
  }
  if (pf->prof_kind.size() <= pf->prof_used) pf->prof_kind.resize(pf->prof_used + 1);
  pf->prof_kind[pf->prof_used] = kind;
  (void)hipEventRecord(pf->prof_ev[pf->prof_used * 2], pf->stream);
}
static inline void prof_end(cssm_pf* pf) {
  if (!pf->profile) return;
  (void)hipEventRecord(pf->prof_ev[pf->prof_used * 2 + 1], pf->stream);
  pf->prof_used++;
}
// after a stream synchronise: fold the recorded pairs into per-kind totals
static inline void prof_collect(cssm_pf* pf) {
  for (size_t i = 0; i < pf->prof_used; ++i) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, pf->prof_ev[2 * i], pf->prof_ev[2 * i + 1]) == hipSuccess) {
      pf->prof_ms[pf->prof_kind[i]] += ms;
      pf->prof_cnt[pf->prof_kind[i]]++;
    }
  }
  pf->prof_used = 0;
}

static inline int grid_for(uint64_t n, int block, int cap) {
  uint64_t g = (n + block - 1) / block;
  if (g > (uint64_t)cap) g = cap;
  if (g < 1) g = 1;
  return (int)g;
}

// The host reads the scalars BEHIND the max slots (err, ess, fail_step, gmax, ref, ll, the sums: ~120 bytes, not the 24 KiB of
// slot lines in front of them -- that copy to pageable memory cost ~15 us per streaming step and per batch call).
#define CSSM_SC_TAIL_OFF offsetof(Scalars, err)
#define CSSM_SC_TAIL_ARGS(hp, scp) reinterpret_cast<char*>(hp) + CSSM_SC_TAIL_OFF, reinterpret_cast<const char*>(scp) + CSSM_SC_TAIL_OFF, sizeof(Scalars) - CSSM_SC_TAIL_OFF

static const int kGridCap = 4096;

#define DISPATCH_D(d, ...)                                                         \
  switch (d) {                                                                      \
    case 1: { constexpr int D = 1; __VA_ARGS__; } break;   case 2: { constexpr int D = 2; __VA_ARGS__; } break;   \
    case 3: { constexpr int D = 3; __VA_ARGS__; } break;   case 4: { constexpr int D = 4; __VA_ARGS__; } break;   \
    case 5: { constexpr int D = 5; __VA_ARGS__; } break;   case 6: { constexpr int D = 6; __VA_ARGS__; } break;   \
    case 7: { constexpr int D = 7; __VA_ARGS__; } break;   case 8: { constexpr int D = 8; __VA_ARGS__; } break;   \
    case 9: { constexpr int D = 9; __VA_ARGS__; } break;   case 10: { constexpr int D = 10; __VA_ARGS__; } break; \
    case 11: { constexpr int D = 11; __VA_ARGS__; } break; case 12: { constexpr int D = 12; __VA_ARGS__; } break; \
    case 13: { constexpr int D = 13; __VA_ARGS__; } break; case 14: { constexpr int D = 14; __VA_ARGS__; } break; \
    case 15: { constexpr int D = 15; __VA_ARGS__; } break; default: { constexpr int D = 16; __VA_ARGS__; } break; \
  }

// ---- defined in cssm_pf.hip, used by cssm_shard.hip as well
int cssm_build_fsub(cssm_pf* pf, size_t first, size_t count, bool reset);   // sub-step table of records [first, +count) -> device
int cssm_ensure_recs(cssm_pf* pf, size_t T);
double cssm_series_t0(const double* t, size_t T);   // the time of a series' initial cloud: its earliest
// records [first, first + count) of a series into h_recs, record s as observation base + s; t_prev: the time before record 0
void cssm_build_recs(cssm_pf* pf, double t_prev, const double* t, const double* y, const uint8_t* has, size_t first, size_t count, uint32_t base);
int cssm_ensure_path(cssm_pf* pf, size_t T);        // d_path holds the T + 1 states of a sampled path
void cssm_note_resampled(cssm_pf* pf, bool optimistic);   // the handle's bookkeeping behind a resampling launch
int cssm_upload_recs(cssm_pf* pf, size_t first, size_t count, bool chain);   // records -> device (+ the predicted level of the first one: LGCP)
int cssm_launch_init(cssm_pf* pf, double t0);
// batched launch (cssm_batch.hip): the chains of the launch; `pf` is chain 0, whose bookkeeping stands for all of them
struct CssmBatchLaunch { const void* chains; int nchains; uint32_t rec_idx; int want_pick; };
int cssm_launch_propagate(cssm_pf* pf, const StepRec* d_rec, double* pick_out = nullptr, uint32_t pick_slot = 0, const CssmBatchLaunch* batch = nullptr);
int cssm_pf_create_on_stream(const cssm_model_desc* desc, uint64_t n_particles, uint64_t seed, int device, hipStream_t stream, cssm_pf** out);
void cssm_batch_fresh(cssm_pf* pf, double t0);   // host-side state of a freshly drawn cloud; the call's generation and completion number
int cssm_check_device_err(cssm_pf* pf, const Scalars& h);
int cssm_use_device(int device);   // the device exists and is current, or the error
double cssm_eta_of_mean(const HostModel& m, const double* fco, const double* mean);   // link(f(stateMean, t)), ParticleFilter.scala:420
void cssm_peer_free(cssm_pf* pf);   // cssm_shard.hip: the peer-written exchange's windows, mappings and device table
// ---- filtered intervals of the single handle: cssm_intervals.hip enqueues the rows, cssm_pf.hip's drivers say when
int cssm_iv_row(cssm_pf* pf, size_t row);        // the summary of the current cloud as row `row` of the running call (8 launches, no host work)
int cssm_iv_results(cssm_pf* pf, size_t nrows);  // behind the call's last launch: its rows on their way to the host
void cssm_iv_free(cssm_pf* pf);
// cssm_pf_ll_filter / cssm_pf_ll_filter_more (cont) with a row behind the initial cloud (not cont) and behind every record; cssm_pf_step with one
// rows: CSSM_ROWS_INTERVALS (cssm_pf_filter_intervals) or CSSM_ROWS_FORECASTS (cssm_pf_filter_forecasts: a row BEFORE every record)
#define CSSM_ROWS_NONE 0
#define CSSM_ROWS_INTERVALS 1
#define CSSM_ROWS_FORECASTS 2
#define CSSM_ROWS_LINEAGE 3      /* cssm_pf_step_interpolate: the step's slice into the window and the lineage rows, enqueued behind the step (after a redo: again) */
int cssm_run_filter_rows(cssm_pf* pf, const double* t, const double* y, const uint8_t* has, size_t T, double* ll_out, double* ll_t, int32_t* ess_t, bool cont,
                         int rows = CSSM_ROWS_INTERVALS);
int cssm_step_rows(cssm_pf* pf, double t, double obs, int has_obs, double* ll_out, int32_t* ess_out, int rows = CSSM_ROWS_INTERVALS);
// ---- one-step-ahead forecasts of the single handle (cssm_pf_filter_forecasts): cssm_intervals.hip holds the rows and the selection,
// cssm_forecast.hip the row's first launch, cssm_pf.hip's drivers say when (before the record's launch_step)
// Scalars::err bits under which every kernel of a row returns at once: a series on hold or waiting for its second run
#define IV_HELD (4u | 8u | 16u | 64u)
int cssm_li_enqueue(cssm_pf* pf);                 // the slice the step just proposed into the window's newest slot, the call's lineage rows, their way to the host
bool cssm_li_has_rows(const cssm_pf* pf);         // whether the running cssm_pf_step_interpolate returns rows (else it only remembers its slice)
int cssm_fc_row(cssm_pf* pf, size_t row);        // the forecast of record `row` of the running call from the cloud as it stands (8 launches, no host work)
int cssm_fc_results(cssm_pf* pf, size_t nrows);
int cssm_forecast_refuse_model(const cssm_pf* pf);   // what cssm_pf_forecast refuses of the handle's model, in its words
int cssm_forecast_row_launch(cssm_pf* pf, const StepRec* d_rec, uint64_t key, double y, int has_y, unsigned long long* keys, double* partial,
                             unsigned long long* pmm, uint32_t* pit, uint32_t* zero, size_t zero_words, unsigned long long* stamp, int nb_f);
